! Test driver: a "host model" that asks for the cloud optical depths its radiation uses, twice - with host arrays dimensioned
! (pcols, .), pcols = ncol + 3, through rrtmg_lw_cloud_optics (module rrtmg_lw_optics), and with fields in device memory from hipMalloc,
! pcols = ncol + 5 wide, the call's columns from column c0 = 4 on, through rrtmg_lw_cloud_optics_dev (module rrtmg_lw_device), passed
! as the elements of the call's first column.  The device output fields hold NaN (ncbands: -1) before the call; the driver counts what
! changed outside the call's columns.  Inputs and outputs travel through stream files written and read by
! tests/test_fortran_cloud_optics.py.
!     drive_cloud_optics <in> <out>
module devmem
  use iso_c_binding
  implicit none
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

program drive_cloud_optics
  use iso_c_binding
  use ieee_arithmetic
  use parkind, only: im => kind_im
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_optics, only: rrtmg_lw_cloud_optics
  use rrtmg_lw_device, only: rrtmg_lw_cloud_optics_dev, rrtmg_lw_dev_check
  use devmem
  implicit none
  integer(im), parameter :: c0 = 4
  integer(im) :: ncol, nlay, imca, inflg, iceflg, liqflg, pcols, pc
  integer :: hdr(6), u, nbad, k
  real(8), allocatable :: cldfr(:,:), taucld(:,:,:), ciwp(:,:), clwp(:,:), rei(:,:), rel(:,:), plev(:,:), h2o(:,:)
  ! the host call: the same arrays dimensioned (pcols, .), and its outputs
  real(8), allocatable :: w_lay(:,:,:), w_tau(:,:,:), w_lev(:,:), o_tau(:,:,:), o_sec(:,:), o_tau2(:,:,:)
  integer(im), allocatable :: o_nb(:)
  ! the device call: host copies of the fields and the fields in device memory - layer arrays (pc,nlay,6) cldfr, cicewp, cliqwp, reice,
  ! reliq, h2ovmr -, taucld (16,pc,nlay), plev (pc,nlay+1), taucloud (pc,nlay,16), secdiff (pc,16), ncbands (pc)
  real(8), allocatable, target :: h_lay(:,:,:), h_tau(:,:,:), h_lev(:,:), h_out(:,:,:), h_sec(:,:)
  integer(c_int32_t), allocatable, target :: h_nb(:)
  type(c_ptr) :: p_lay, p_tau, p_lev, p_out, p_sec, p_nb
  real(8), pointer, contiguous :: lay(:,:,:), tau(:,:,:), lev(:,:), out(:,:,:), sec(:,:)
  integer(c_int32_t), pointer, contiguous :: nb(:)
  real(8) :: nan
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr
  ncol = hdr(1); nlay = hdr(2); imca = hdr(3); inflg = hdr(4); iceflg = hdr(5); liqflg = hdr(6)
  allocate(cldfr(ncol,nlay), taucld(16,ncol,nlay), ciwp(ncol,nlay), clwp(ncol,nlay), rei(ncol,nlay), rel(ncol,nlay), plev(ncol,nlay+1), h2o(ncol,nlay))
  read(u) cldfr, taucld, ciwp, clwp, rei, rel, plev, h2o
  close(u)
  nan = ieee_value(nan, ieee_quiet_nan)
  call rrtmg_lw_ini(1004.0_8)

  ! ---- host arrays larger than the call (pcols > ncol): the rest holds NaN
  pcols = ncol + 3
  allocate(w_lay(pcols,nlay,6), w_tau(16,pcols,nlay), w_lev(pcols,nlay+1), o_tau(pcols,nlay,16), o_sec(pcols,16), o_nb(pcols), o_tau2(ncol,nlay,16))
  w_lay = nan; w_tau = nan; w_lev = nan; o_tau = nan; o_sec = nan; o_nb = -1
  w_lay(1:ncol,:,1) = cldfr; w_lay(1:ncol,:,2) = ciwp; w_lay(1:ncol,:,3) = clwp; w_lay(1:ncol,:,4) = rei; w_lay(1:ncol,:,5) = rel
  w_lay(1:ncol,:,6) = h2o; w_tau(:,1:ncol,:) = taucld; w_lev(1:ncol,:) = plev
  call rrtmg_lw_cloud_optics(ncol, nlay, imca, inflg, iceflg, liqflg, w_lay(:,:,1), w_tau, w_lay(:,:,2), w_lay(:,:,3), w_lay(:,:,4), &
                             w_lay(:,:,5), plev=w_lev, h2ovmr=w_lay(:,:,6), taucloud=o_tau, ncbands=o_nb, secdiff=o_sec)
  ! ... and one output alone, exactly sized, by keyword
  call rrtmg_lw_cloud_optics(ncol, nlay, imca, inflg, iceflg, liqflg, cldfr, taucld, ciwp, clwp, rei, rel, taucloud=o_tau2)
  nbad = count(.not. ieee_is_nan(o_tau(ncol+1:,:,:))) + count(.not. ieee_is_nan(o_sec(ncol+1:,:))) + count(o_nb(ncol+1:) /= -1)
  if (any(o_tau2 /= o_tau(1:ncol,:,:))) nbad = nbad + 1000000

  ! ---- device fields
  pc = ncol + 5
  allocate(h_lay(pc,nlay,6), h_tau(16,pc,nlay), h_lev(pc,nlay+1), h_out(pc,nlay,16), h_sec(pc,16), h_nb(pc))
  h_lay = nan; h_tau = nan; h_lev = nan; h_out = nan; h_sec = nan; h_nb = -1
  h_lay(c0:c0+ncol-1,:,:) = w_lay(1:ncol,:,:); h_tau(:,c0:c0+ncol-1,:) = taucld; h_lev(c0:c0+ncol-1,:) = plev
  call upload(c_loc(h_lay), int(size(h_lay), c_size_t) * 8, p_lay)
  call upload(c_loc(h_tau), int(size(h_tau), c_size_t) * 8, p_tau)
  call upload(c_loc(h_lev), int(size(h_lev), c_size_t) * 8, p_lev)
  call upload(c_loc(h_out), int(size(h_out), c_size_t) * 8, p_out)
  call upload(c_loc(h_sec), int(size(h_sec), c_size_t) * 8, p_sec)
  call upload(c_loc(h_nb), int(size(h_nb), c_size_t) * 4, p_nb)
  call c_f_pointer(p_lay, lay, [pc, nlay, 6_im]); call c_f_pointer(p_tau, tau, [16_im, pc, nlay]); call c_f_pointer(p_lev, lev, [pc, nlay + 1])
  call c_f_pointer(p_out, out, [pc, nlay, 16_im]); call c_f_pointer(p_sec, sec, [pc, 16_im]); call c_f_pointer(p_nb, nb, [pc])
  ! (the dummies are never touched on the host: every actual below is a device address)
  call rrtmg_lw_cloud_optics_dev(ncol, pc, nlay, imca, inflg, iceflg, liqflg, lay(c0,1,1), tau(1,c0,1), lay(c0,1,2), lay(c0,1,3), &
                                 lay(c0,1,4), lay(c0,1,5), plev=lev(c0,1), h2ovmr=lay(c0,1,6), taucloud=out(c0,1,1), ncbands=nb(c0), &
                                 secdiff=sec(c0,1))
  call rrtmg_lw_dev_check()
  call download(c_loc(h_out), int(size(h_out), c_size_t) * 8, p_out)
  call download(c_loc(h_sec), int(size(h_sec), c_size_t) * 8, p_sec)
  call download(c_loc(h_nb), int(size(h_nb), c_size_t) * 4, p_nb)
  do k = 1, int(pc)
     if (k >= c0 .and. k < c0 + ncol) cycle
     nbad = nbad + count(.not. ieee_is_nan(h_out(k,:,:))) + count(.not. ieee_is_nan(h_sec(k,:)))
     if (h_nb(k) /= -1) nbad = nbad + 1
  enddo
  call need(hipFree(p_lay), 'hipFree'); call need(hipFree(p_tau), 'hipFree'); call need(hipFree(p_lev), 'hipFree')
  call need(hipFree(p_out), 'hipFree'); call need(hipFree(p_sec), 'hipFree'); call need(hipFree(p_nb), 'hipFree')

  ! nbad, 0; the host call's taucloud, secdiff, ncbands; the device call's
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) nbad, 0
  write(u) o_tau(1:ncol,:,:), o_sec(1:ncol,:), int(o_nb(1:ncol), 4)
  write(u) h_out(c0:c0+ncol-1,:,:), h_sec(c0:c0+ncol-1,:), h_nb(c0:c0+ncol-1)
  close(u)
end program drive_cloud_optics
