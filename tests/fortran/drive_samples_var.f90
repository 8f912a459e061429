! Test driver: tests/fortran/drive_samples.f90 with the optional sample variances of module rrtmg_lw_samples - hr_var by keyword alone
! first (the other two absent), then all three; the stream files are those of tests/test_fortran_samples_dev.py.  Output: icld, the
! eight outputs of the second call, uflx_var, dflx_var, hr_var, and hr_var of the first call.
program drive_samples_var
  use parkind, only: im => kind_im, rb => kind_rb
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_samples, only: rrtmg_lw_mcica_samples
  implicit none
  integer(im) :: ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, inflg, iceflg, liqflg
  integer :: hdr(11), u, v
  real(rb), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), gas(:,:,:), emis(:,:), cld(:,:,:), alpha(:,:)
  real(rb), allocatable :: taucld(:,:,:), tauaer(:,:,:)
  real(rb), allocatable :: uflx(:,:), dflx(:,:), hr(:,:), uflxc(:,:), dflxc(:,:), hrc(:,:), duflx_dt(:,:), duflxc_dt(:,:)
  real(rb), allocatable :: uflx_var(:,:), dflx_var(:,:), hr_var(:,:), hr_var_alone(:,:)
  integer(im) :: icld_in
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
  allocate(uflx_var(ncol,nlay+1), dflx_var(ncol,nlay+1), hr_var(ncol,nlay), hr_var_alone(ncol,nlay))
  read(u) play, plev, tlay, tlev, tsfc, gas, emis, cld, alpha, taucld, tauaer
  close(u)
  duflx_dt = 0._rb; duflxc_dt = 0._rb
  call rrtmg_lw_ini(1004.0_rb)
  icld_in = icld
  call rrtmg_lw_mcica_samples(ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, plev, tlay, tlev, tsfc, &
        gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), gas(:,:,5), gas(:,:,6), gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), &
        emis, inflg, iceflg, liqflg, cld(:,:,1), taucld, cld(:,:,2), cld(:,:,3), cld(:,:,4), cld(:,:,5), alpha, tauaer, &
        uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, hr_var=hr_var_alone)
  icld = icld_in
  call rrtmg_lw_mcica_samples(ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, plev, tlay, tlev, tsfc, &
        gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), gas(:,:,5), gas(:,:,6), gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), &
        emis, inflg, iceflg, liqflg, cld(:,:,1), taucld, cld(:,:,2), cld(:,:,3), cld(:,:,4), cld(:,:,5), alpha, tauaer, &
        uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var)
  open(newunit=v, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(v) int(icld, 4)
  write(v) uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt
  write(v) uflx_var, dflx_var, hr_var, hr_var_alone
  close(v)
end program drive_samples_var
