! Test driver: a "host model" that adjusts stored idrv = 1 fluxes to a changed surface temperature (module rrtmg_lw_adjust), for every
! case of a stream file written by tests/test_adjust_tsfc.py: once with the optional clear-sky arguments, once without them (hr_adj then
! oversized, dimensioned with pcols > ncol: through the shim's temporary).  Results go to a second stream file, case by case.
program drive_adjust
  use parkind, only: im => kind_im, rb => kind_rb
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_adjust, only: rrtmg_lw_dtsfc
  implicit none
  integer(im) :: ncol, nlay, pcols
  integer :: ncase, hdr(2), u, v, ic
  real(rb), allocatable :: plev(:,:), dtsfc(:), uflx(:,:), dflx(:,:), duflx_dt(:,:), uflxc(:,:), dflxc(:,:), duflxc_dt(:,:)
  real(rb), allocatable :: ua(:,:), hr(:,:), uca(:,:), hrc(:,:), ua2(:,:), hr2(:,:)
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  open(newunit=v, file=trim(fout), access='stream', form='unformatted', status='replace')
  call rrtmg_lw_ini(1004.0_rb)
  read(u) ncase
  do ic = 1, ncase
     read(u) hdr
     ncol = hdr(1); nlay = hdr(2); pcols = ncol + 3
     allocate(plev(ncol,nlay+1), dtsfc(ncol), uflx(ncol,nlay+1), dflx(ncol,nlay+1), duflx_dt(ncol,nlay+1))
     allocate(uflxc(ncol,nlay+1), dflxc(ncol,nlay+1), duflxc_dt(ncol,nlay+1))
     allocate(ua(ncol,nlay+1), hr(ncol,nlay), uca(ncol,nlay+1), hrc(ncol,nlay), ua2(ncol,nlay+1), hr2(pcols,nlay))
     read(u) plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt
     hr2 = -1._rb
     call rrtmg_lw_dtsfc(ncol, nlay, plev, dtsfc, uflx, dflx, duflx_dt, ua, hr, &
                         uflxc=uflxc, dflxc=dflxc, duflxc_dt=duflxc_dt, uflxc_adj=uca, hrc_adj=hrc)
     call rrtmg_lw_dtsfc(ncol, nlay, plev, dtsfc, uflx, dflx, duflx_dt, ua2, hr2)
     if (any(hr2(ncol+1:pcols,:) /= -1._rb)) then
        write(*,*) 'drive_adjust: columns beyond ncol were written'
        error stop 2
     endif
     write(v) ua, hr, uca, hrc, ua2, hr2(1:ncol,:)
     deallocate(plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt, ua, hr, uca, hrc, ua2, hr2)
  enddo
  close(u)
  close(v)
end program drive_adjust
