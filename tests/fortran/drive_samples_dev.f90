! Test driver: a GPU-resident "host model" that averages sub-column samples.  As tests/fortran/drive_device.f90: fields in device memory
! from hipMalloc, dimensioned (pcols, .) with pcols = ncol + 5, the call's columns from column c0 = 4 on and NaN everywhere else, passed
! to module rrtmg_lw_device as the elements of the call's first column.  It forms alpha on the device (rrtmg_lw_alpha_dev) and hands it
! straight to rrtmg_lw_mcica_samples_dev, which returns the means and the three sample variances.
! Compiled with -cpp; -DWP=4 makes it a host built with 4-byte reals.  Inputs and outputs travel through stream files written and read
! by tests/test_fortran_samples_dev.py (always float64 in the files).
!     drive_samples_dev <in> <out>
#ifndef WP
#define WP 8
#endif
module devmem
  use iso_c_binding
  implicit none
  integer, parameter :: wp = WP
  integer(c_int), parameter :: H2D = 1, D2H = 2
  interface
     function hipMalloc(p, bytes) bind(C, name='hipMalloc') result(rc)
       import :: c_ptr, c_size_t, c_int
       type(c_ptr), intent(out) :: p
       integer(c_size_t), value :: bytes
       integer(c_int) :: rc
     end function hipMalloc
     function hipMemcpy(dst, src, bytes, kind) bind(C, name='hipMemcpy') result(rc)
       import :: c_ptr, c_size_t, c_int
       type(c_ptr), value :: dst, src
       integer(c_size_t), value :: bytes
       integer(c_int), value :: kind
       integer(c_int) :: rc
     end function hipMemcpy
     function hipFree(p) bind(C, name='hipFree') result(rc)
       import :: c_ptr, c_int
       type(c_ptr), value :: p
       integer(c_int) :: rc
     end function hipFree
     function hipStreamCreate(s) bind(C, name='hipStreamCreate') result(rc)
       import :: c_ptr, c_int
       type(c_ptr), intent(out) :: s
       integer(c_int) :: rc
     end function hipStreamCreate
     function hipStreamDestroy(s) bind(C, name='hipStreamDestroy') result(rc)
       import :: c_ptr, c_int
       type(c_ptr), value :: s
       integer(c_int) :: rc
     end function hipStreamDestroy
  end interface
contains
  subroutine need(rc, what)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: what
    if (rc /= 0) then
       write(*,'(a,a,i0)') what, ' failed: ', rc
       error stop 1
    endif
  end subroutine need
  ! a device field of n values holding the host array h
  subroutine upload(h, n, d)
    real(wp), intent(in), target :: h(*)
    integer, intent(in) :: n
    type(c_ptr), intent(out) :: d
    call need(hipMalloc(d, int(n, c_size_t) * WP), 'hipMalloc')
    call need(hipMemcpy(d, c_loc(h), int(n, c_size_t) * WP, H2D), 'hipMemcpy')
  end subroutine upload
  subroutine download(h, n, d)
    real(wp), intent(out), target :: h(*)
    integer, intent(in) :: n
    type(c_ptr), intent(in) :: d
    call need(hipMemcpy(c_loc(h), d, int(n, c_size_t) * WP, D2H), 'hipMemcpy')
  end subroutine download
end module devmem

program drive_samples_dev
  use iso_c_binding
  use ieee_arithmetic
  use parkind, only: im => kind_im
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_device, only: rrtmg_lw_mcica_samples_dev, rrtmg_lw_alpha_dev, rrtmg_lw_dev_check
  use devmem
  implicit none
  integer(im), parameter :: c0 = 4
  integer(im) :: ncol, nlay, icld, icld_gen, idrv, inflg, iceflg, liqflg, pcols, seed, nsamp, seedstep, idcor, juldat, irng
  integer :: hdr(12), u, nbad, k
  real(8) :: decorr_con
  real(8), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), gas(:,:,:), emis(:,:)
  real(8), allocatable :: cld(:,:,:), taucld(:,:,:), tauaer(:,:,:), dz(:,:), lat(:)
  ! the host's copies of its fields (pcols wide) and the fields themselves, in device memory
  real(wp), allocatable, target :: h_lay(:,:,:), h_lev(:,:,:), h_col(:,:), h_emis(:,:), h_taucld(:,:,:), h_tauaer(:,:,:)
  real(wp), allocatable, target :: h_olev(:,:,:), h_olay(:,:,:)
  type(c_ptr) :: p_lay, p_lev, p_col, p_emis, p_taucld, p_tauaer, p_olev, p_olay, stream
  real(wp), pointer, contiguous :: lay(:,:,:), lev(:,:,:), col(:,:), demis(:,:), dtaucld(:,:,:), dtauaer(:,:,:)
  real(wp), pointer, contiguous :: olev(:,:,:), olay(:,:,:)
  real(wp) :: nan
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr, decorr_con
  ncol = hdr(1); nlay = hdr(2); icld = hdr(3); idrv = hdr(4); inflg = hdr(5); iceflg = hdr(6); liqflg = hdr(7); seed = hdr(8)
  nsamp = hdr(9); seedstep = hdr(10); idcor = hdr(11); juldat = hdr(12)
  pcols = ncol + 5
  allocate(play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol), gas(ncol,nlay,10))
  allocate(emis(ncol,16), cld(ncol,nlay,5), taucld(16,ncol,nlay), tauaer(ncol,nlay,16), dz(ncol,nlay), lat(ncol))
  read(u) play, plev, tlay, tlev, tsfc, gas, emis, cld, taucld, tauaer, dz, lat
  close(u)

  ! the fields: layer arrays (pcols,nlay,19): play, tlay, the ten gases, the five cloud arrays, dz, alpha (made on the device); level
  ! arrays (pcols,nlay+1,2): plev, tlev; per-column values (pcols,2): tsfc, lat.  NaN outside the call's columns, and in all of alpha.
  nan = ieee_value(nan, ieee_quiet_nan)
  allocate(h_lay(pcols,nlay,19), h_lev(pcols,nlay+1,2), h_col(pcols,2), h_emis(pcols,16), h_taucld(16,pcols,nlay), h_tauaer(pcols,nlay,16))
  h_lay = nan; h_lev = nan; h_col = nan; h_emis = nan; h_taucld = nan; h_tauaer = nan
  h_lay(c0:c0+ncol-1,:,1) = real(play, wp); h_lay(c0:c0+ncol-1,:,2) = real(tlay, wp)
  h_lay(c0:c0+ncol-1,:,3:12) = real(gas, wp); h_lay(c0:c0+ncol-1,:,13:17) = real(cld, wp)
  h_lay(c0:c0+ncol-1,:,18) = real(dz, wp)
  h_lev(c0:c0+ncol-1,:,1) = real(plev, wp); h_lev(c0:c0+ncol-1,:,2) = real(tlev, wp)
  h_col(c0:c0+ncol-1,1) = real(tsfc, wp); h_col(c0:c0+ncol-1,2) = real(lat, wp)
  h_emis(c0:c0+ncol-1,:) = real(emis, wp)
  h_taucld(:,c0:c0+ncol-1,:) = real(taucld, wp)
  h_tauaer(c0:c0+ncol-1,:,:) = real(tauaer, wp)
  ! outputs: level arrays (pcols,nlay+1,8): uflx, dflx, uflxc, dflxc, duflx_dt, duflxc_dt, uflx_var, dflx_var; layer arrays
  ! (pcols,nlay,3): hr, hrc, hr_var.  NaN everywhere.
  allocate(h_olev(pcols,nlay+1,8), h_olay(pcols,nlay,3))
  h_olev = nan; h_olay = nan

  call rrtmg_lw_ini(1004.0_8)
  call upload(h_lay, size(h_lay), p_lay); call upload(h_lev, size(h_lev), p_lev); call upload(h_col, size(h_col), p_col)
  call upload(h_emis, size(h_emis), p_emis); call upload(h_taucld, size(h_taucld), p_taucld); call upload(h_tauaer, size(h_tauaer), p_tauaer)
  call upload(h_olev, size(h_olev), p_olev); call upload(h_olay, size(h_olay), p_olay)
  call c_f_pointer(p_lay, lay, [pcols, nlay, 19_im]); call c_f_pointer(p_lev, lev, [pcols, nlay+1, 2_im]); call c_f_pointer(p_col, col, [pcols, 2_im])
  call c_f_pointer(p_emis, demis, [pcols, 16_im]); call c_f_pointer(p_taucld, dtaucld, [16_im, pcols, nlay])
  call c_f_pointer(p_tauaer, dtauaer, [pcols, nlay, 16_im])
  call c_f_pointer(p_olev, olev, [pcols, nlay+1, 8_im]); call c_f_pointer(p_olay, olay, [pcols, nlay, 3_im])
  call need(hipStreamCreate(stream), 'hipStreamCreate')

  ! (the dummies are never touched on the host: every actual below is a device address)
  icld_gen = icld
  irng = 0
  call rrtmg_lw_alpha_dev(ncol, pcols, nlay, icld_gen, idcor, real(decorr_con, wp), lay(c0,1,18), col(c0,2), juldat, lay(c0,1,13), &
                          lay(c0,1,19), stream)
  call rrtmg_lw_mcica_samples_dev(ncol, pcols, nlay, icld, idrv, seed, nsamp, seedstep, irng, &
                    lay(c0,1,1), lev(c0,1,1), lay(c0,1,2), lev(c0,1,2), col(c0,1), &
                    lay(c0,1,3), lay(c0,1,4), lay(c0,1,5), lay(c0,1,6), lay(c0,1,7), lay(c0,1,8), &
                    lay(c0,1,9), lay(c0,1,10), lay(c0,1,11), lay(c0,1,12), demis(c0,1), inflg, iceflg, liqflg, &
                    lay(c0,1,13), dtaucld(1,c0,1), lay(c0,1,14), lay(c0,1,15), lay(c0,1,16), lay(c0,1,17), lay(c0,1,19), dtauaer(c0,1,1), &
                    olev(c0,1,1), olev(c0,1,2), olay(c0,1,1), olev(c0,1,3), olev(c0,1,4), olay(c0,1,2), &
                    olev(c0,1,5), olev(c0,1,6), olev(c0,1,7), olev(c0,1,8), olay(c0,1,3), stream)
  call rrtmg_lw_dev_check(stream)

  call download(h_olev, size(h_olev), p_olev); call download(h_olay, size(h_olay), p_olay); call download(h_lay, size(h_lay), p_lay)
  ! nothing outside the call's columns may have been written: those elements still hold NaN
  nbad = 0
  do k = 1, int(pcols)
     if (k >= c0 .and. k < c0 + ncol) cycle
     nbad = nbad + count(.not. ieee_is_nan(h_olev(k,:,:))) + count(.not. ieee_is_nan(h_olay(k,:,:))) + count(.not. ieee_is_nan(h_lay(k,:,19)))
  enddo
  call need(hipStreamDestroy(stream), 'hipStreamDestroy')
  call need(hipFree(p_lay), 'hipFree'); call need(hipFree(p_lev), 'hipFree'); call need(hipFree(p_col), 'hipFree')
  call need(hipFree(p_emis), 'hipFree'); call need(hipFree(p_taucld), 'hipFree'); call need(hipFree(p_tauaer), 'hipFree')
  call need(hipFree(p_olev), 'hipFree'); call need(hipFree(p_olay), 'hipFree')

  ! icld, nbad, then float64: uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, alpha
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) int(icld), nbad
  write(u) real(h_olev(c0:c0+ncol-1,:,1), 8), real(h_olev(c0:c0+ncol-1,:,2), 8), real(h_olay(c0:c0+ncol-1,:,1), 8)
  write(u) real(h_olev(c0:c0+ncol-1,:,3), 8), real(h_olev(c0:c0+ncol-1,:,4), 8), real(h_olay(c0:c0+ncol-1,:,2), 8)
  write(u) real(h_olev(c0:c0+ncol-1,:,5), 8), real(h_olev(c0:c0+ncol-1,:,6), 8)
  write(u) real(h_olev(c0:c0+ncol-1,:,7), 8), real(h_olev(c0:c0+ncol-1,:,8), 8), real(h_olay(c0:c0+ncol-1,:,3), 8)
  write(u) real(h_lay(c0:c0+ncol-1,:,19), 8)
  close(u)
end program drive_samples_dev
