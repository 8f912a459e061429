! Test driver: a GPU-resident "host model" that diagnoses cloud cover from the sub-columns its radiation sees.  As
! tests/fortran/drive_samples_dev.f90: fields in device memory from hipMalloc, dimensioned (pcols, .) with pcols = ncol + 5, the call's
! columns from column c0 = 4 on, passed to rrtmg_lw_cloud_cover_dev (module rrtmg_lw_device) as the elements of the call's first column.
! The output fields hold NaN (the mask: -1) everywhere before the call; the driver counts what changed outside the call's columns.
! Compiled with -cpp; -DWP=4 makes it a host built with 4-byte reals.  Inputs and outputs travel through stream files written and read
! by tests/test_fortran_cloud_cover.py (always float64 in the files).
!     drive_cloud_cover_dev <in> <out>
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
  ! a device field of `bytes` bytes holding what lies at the host address h
  subroutine upload(h, bytes, d)
    type(c_ptr), intent(in) :: h
    integer(c_size_t), intent(in) :: bytes
    type(c_ptr), intent(out) :: d
    call need(hipMalloc(d, bytes), 'hipMalloc')
    call need(hipMemcpy(d, h, bytes, H2D), 'hipMemcpy')
  end subroutine upload
  subroutine download(h, bytes, d)
    type(c_ptr), intent(in) :: h, d
    integer(c_size_t), intent(in) :: bytes
    call need(hipMemcpy(h, d, bytes, D2H), 'hipMemcpy')
  end subroutine download
end module devmem

program drive_cloud_cover_dev
  use iso_c_binding
  use ieee_arithmetic
  use parkind, only: im => kind_im
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_device, only: rrtmg_lw_cloud_cover_dev, rrtmg_lw_dev_check
  use devmem
  implicit none
  integer(im), parameter :: c0 = 4, mw = 5
  integer(im) :: ncol, nlay, icld, seed, nsamp, seedstep, irng, pcols
  integer :: hdr(7), u, nbad, k
  real(8), allocatable :: play(:,:), cldfr(:,:), alpha(:,:)
  ! the host's copies of its fields (pcols wide) and the fields themselves, in device memory: layer arrays (pcols,nlay,5) - play, cldfr,
  ! alpha, cldcum, cldlay -, the per-column cldtot (pcols), the mask (pcols,nlay,mw)
  real(wp), allocatable, target :: h_lay(:,:,:), h_col(:)
  integer(c_int32_t), allocatable, target :: h_mask(:,:,:)
  type(c_ptr) :: p_lay, p_col, p_mask
  real(wp), pointer, contiguous :: lay(:,:,:), col(:)
  integer(c_int32_t), pointer, contiguous :: mask(:,:,:)
  real(wp) :: nan
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr
  ncol = hdr(1); nlay = hdr(2); icld = hdr(3); seed = hdr(4); nsamp = hdr(5); seedstep = hdr(6); irng = hdr(7)
  pcols = ncol + 5
  allocate(play(ncol,nlay), cldfr(ncol,nlay), alpha(ncol,nlay))
  read(u) play, cldfr, alpha
  close(u)

  nan = ieee_value(nan, ieee_quiet_nan)
  allocate(h_lay(pcols,nlay,5), h_col(pcols), h_mask(pcols,nlay,mw))
  h_lay = nan; h_col = nan; h_mask = -1
  h_lay(c0:c0+ncol-1,:,1) = real(play, wp); h_lay(c0:c0+ncol-1,:,2) = real(cldfr, wp); h_lay(c0:c0+ncol-1,:,3) = real(alpha, wp)

  call rrtmg_lw_ini(1004.0_8)
  call upload(c_loc(h_lay), int(size(h_lay), c_size_t) * WP, p_lay)
  call upload(c_loc(h_col), int(size(h_col), c_size_t) * WP, p_col)
  call upload(c_loc(h_mask), int(size(h_mask), c_size_t) * 4, p_mask)
  call c_f_pointer(p_lay, lay, [pcols, nlay, 5_im]); call c_f_pointer(p_col, col, [pcols]); call c_f_pointer(p_mask, mask, [pcols, nlay, mw])

  ! (the dummies are never touched on the host: every actual below is a device address)
  if (nsamp == 1) then
     call rrtmg_lw_cloud_cover_dev(ncol, pcols, nlay, icld, seed, nsamp, seedstep, irng, lay(c0,1,1), lay(c0,1,2), lay(c0,1,3), &
                                   col(c0), lay(c0,1,4), lay(c0,1,5), mask(c0,1,1))
  else
     call rrtmg_lw_cloud_cover_dev(ncol, pcols, nlay, icld, seed, nsamp, seedstep, irng, lay(c0,1,1), lay(c0,1,2), alpha=lay(c0,1,3), &
                                   cldtot=col(c0), cldcum=lay(c0,1,4), cldlay=lay(c0,1,5))
  endif
  call rrtmg_lw_dev_check()

  call download(c_loc(h_lay), int(size(h_lay), c_size_t) * WP, p_lay)
  call download(c_loc(h_col), int(size(h_col), c_size_t) * WP, p_col)
  call download(c_loc(h_mask), int(size(h_mask), c_size_t) * 4, p_mask)
  ! nothing outside the call's columns may have been written: those elements still hold NaN, those mask words -1
  nbad = 0
  do k = 1, int(pcols)
     if (k >= c0 .and. k < c0 + ncol) cycle
     nbad = nbad + count(.not. ieee_is_nan(h_lay(k,:,4:5))) + count(h_mask(k,:,:) /= -1)
     if (.not. ieee_is_nan(h_col(k))) nbad = nbad + 1
  enddo
  call need(hipFree(p_lay), 'hipFree'); call need(hipFree(p_col), 'hipFree'); call need(hipFree(p_mask), 'hipFree')

  ! irng, nbad, then float64: cldtot, cldcum, cldlay; then the mask words of the call's columns
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) int(irng, 4), nbad
  write(u) real(h_col(c0:c0+ncol-1), 8), real(h_lay(c0:c0+ncol-1,:,4), 8), real(h_lay(c0:c0+ncol-1,:,5), 8)
  write(u) h_mask(c0:c0+ncol-1,:,:)
  close(u)
end program drive_cloud_cover_dev
