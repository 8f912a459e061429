! Test driver: a "host model" that asks rrtmg_lw (non-McICA shim) for the fluxes per band through the optional dummies uflxs, dflxs,
! uflxcs, dflxcs.  The total-sky ones are exactly sized (passed in place), the clear-sky ones oversized - dimensioned (pcols, nlay+1, 16)
! with pcols > ncol, as a host with a fixed chunk width keeps them - and go through the shim's temporaries.  Inputs from a stream file
! written by tests/test_fortran_spectral.py (the layout of drive_shim.f90).
program drive_spectral
  use parkind, only: im => kind_im, rb => kind_rb
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_rad, only: rrtmg_lw
  implicit none
  integer(im) :: ncol, nlay, icld, idrv, inflg, iceflg, liqflg, pcols
  integer :: hdr(7), u
  real(rb), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), gas(:,:,:), emis(:,:)
  real(rb), allocatable :: cld(:,:,:), taucld(:,:,:), tauaer(:,:,:)
  real(rb), allocatable :: uflx(:,:), dflx(:,:), hr(:,:), uflxc(:,:), dflxc(:,:), hrc(:,:), du(:,:), duc(:,:)
  real(rb), allocatable :: us(:,:,:), ds(:,:,:), ucs(:,:,:), dcs(:,:,:)
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr
  ncol = hdr(1); nlay = hdr(2); icld = hdr(3); idrv = hdr(4); inflg = hdr(5); iceflg = hdr(6); liqflg = hdr(7)
  allocate(play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol), gas(ncol,nlay,10))
  allocate(emis(ncol,16), cld(ncol,nlay,5), taucld(16,ncol,nlay), tauaer(ncol,nlay,16))
  read(u) play, plev, tlay, tlev, tsfc, gas, emis, cld, taucld, tauaer
  close(u)
  allocate(uflx(ncol,nlay+1), dflx(ncol,nlay+1), hr(ncol,nlay), uflxc(ncol,nlay+1), dflxc(ncol,nlay+1), hrc(ncol,nlay))
  allocate(du(ncol,nlay+1), duc(ncol,nlay+1))
  pcols = ncol + 3
  allocate(us(ncol,nlay+1,16), ds(ncol,nlay+1,16), ucs(pcols,nlay+1,16), dcs(pcols,nlay+1,16))
  du = 0._rb; duc = 0._rb
  us = -1._rb; ds = -1._rb; ucs = -1._rb; dcs = -1._rb

  call rrtmg_lw_ini(1004.0_rb)
  call rrtmg_lw(ncol, nlay, icld, idrv, play, plev, tlay, tlev, tsfc, &
                gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), gas(:,:,5), gas(:,:,6), &
                gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), emis, inflg, iceflg, liqflg, &
                cld(:,:,1), taucld, cld(:,:,2), cld(:,:,3), cld(:,:,4), cld(:,:,5), tauaer, &
                uflx, dflx, hr, uflxc, dflxc, hrc, du, duc, &
                uflxs=us, dflxs=ds, uflxcs=ucs, dflxcs=dcs)
  if (any(ucs(ncol+1:pcols,:,:) /= -1._rb) .or. any(dcs(ncol+1:pcols,:,:) /= -1._rb)) then
     write(*,*) 'drive_spectral: columns beyond ncol were written'
     error stop 2
  endif
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) int(icld), uflx, dflx, hr, uflxc, dflxc, hrc, us, ds, ucs(1:ncol,:,:), dcs(1:ncol,:,:)
  close(u)
end program drive_spectral
