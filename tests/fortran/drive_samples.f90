! Test driver: a "host model" that asks for the mean over several sub-column samples (module rrtmg_lw_samples) with the arrays of a
! stream file written by tests/test_fortran_samples.py; icld as it comes back and the eight outputs go to a second stream file.
program drive_samples
  use parkind, only: im => kind_im, rb => kind_rb
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_samples, only: rrtmg_lw_mcica_samples
  implicit none
  integer(im) :: ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, inflg, iceflg, liqflg
  integer :: hdr(11), u, v
  real(rb), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), gas(:,:,:), emis(:,:), cld(:,:,:), alpha(:,:)
  real(rb), allocatable :: taucld(:,:,:), tauaer(:,:,:)
  real(rb), allocatable :: uflx(:,:), dflx(:,:), hr(:,:), uflxc(:,:), dflxc(:,:), hrc(:,:), duflx_dt(:,:), duflxc_dt(:,:)
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr
  ncol = hdr(1); nlay = hdr(2); icld = hdr(3); idrv = hdr(4); inflg = hdr(5); iceflg = hdr(6); liqflg = hdr(7)
  permuteseed = hdr(8); nsamp = hdr(9); seedstep = hdr(10); irng = hdr(11)
  allocate(play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol), gas(ncol,nlay,10), emis(ncol,16))
  allocate(cld(ncol,nlay,5), alpha(ncol,nlay), taucld(16,ncol,nlay), tauaer(ncol,nlay,16))
  allocate(uflx(ncol,nlay+1), dflx(ncol,nlay+1), hr(ncol,nlay), uflxc(ncol,nlay+1), dflxc(ncol,nlay+1), hrc(ncol,nlay))
  allocate(duflx_dt(ncol,nlay+1), duflxc_dt(ncol,nlay+1))
  read(u) play, plev, tlay, tlev, tsfc, gas, emis, cld, alpha, taucld, tauaer
  close(u)
  duflx_dt = 0._rb; duflxc_dt = 0._rb
  call rrtmg_lw_ini(1004.0_rb)
  call rrtmg_lw_mcica_samples(ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, plev, tlay, tlev, tsfc, &
        gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), gas(:,:,5), gas(:,:,6), gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), &
        emis, inflg, iceflg, liqflg, cld(:,:,1), taucld, cld(:,:,2), cld(:,:,3), cld(:,:,4), cld(:,:,5), alpha, tauaer, &
        uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt)
  open(newunit=v, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(v) int(icld, 4)
  write(v) uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt
  close(v)
end program drive_samples
