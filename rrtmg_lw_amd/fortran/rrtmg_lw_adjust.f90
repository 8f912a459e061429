!  Surface-temperature adjustment of idrv = 1 results (this library's extension; include/rrtmg_lw_hip.h, "Surface-temperature adjustment"):
!      use rrtmg_lw_adjust, only: rrtmg_lw_dtsfc
!      call rrtmg_lw_dtsfc(ncol, nlay, plev, dtsfc, uflx, dflx, duflx_dt, uflx_adj, hr_adj &
!                          [, uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj])
!  What the reference's column driver does after an idrv = 1 call (src/rrtmg_lw.1col.f90:582-610), for the GCM interface: with
!  uflx, dflx, duflx_dt (ncol,nlay+1) as rrtmg_lw (module rrtmg_lw_rad) returned them and dtsfc (ncol) = the current surface temperature
!  minus the tsfc of that call,
!      uflx_adj (ncol,nlay+1) = uflx + duflx_dt * dtsfc       hr_adj (ncol,nlay): the heating rate of the new net flux (K/day)
!  The inputs are always the stored results of the radiation call, on every step between two calls; downward fluxes do not change.
!  The five clear-sky arguments are optional: all present or all absent.  Arrays larger than the declared shapes (pcols > ncol) or
!  strided sections are accepted as in rrtmg_lw_rad: they go across as the section (1:ncol, ...), through temporaries where they are
!  not exactly sized.  rrtmg_lw_dtsfc is generic over the real kind: real(4) arrays (a host built with 4-byte reals) go to
!  rrtmg_lw_hip_adjust_tsfc_r4 - the arithmetic in float64 on the widened values, the results rounded.
      module rrtmg_lw_adjust

      use iso_c_binding
      use parkind, only : im => kind_im, rb => kind_rb
      use rrtmg_lw_init, only : rrtmg_lw_hip_abort

      implicit none

      public :: rrtmg_lw_dtsfc

      integer, parameter, private :: r4 = c_float

      interface rrtmg_lw_dtsfc
         module procedure rrtmg_lw_dtsfc_r8, rrtmg_lw_dtsfc_r4
      end interface

      interface
         function rrtmg_lw_hip_adjust_tsfc(ncol, nlay, plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt, &
               uflx_adj, hr_adj, uflxc_adj, hrc_adj) bind(C, name='rrtmg_lw_hip_adjust_tsfc') result(rc)
            import :: c_int, c_double, c_ptr
            integer(c_int), value :: ncol, nlay
            real(c_double), intent(in) :: plev(*), dtsfc(*), uflx(*), dflx(*), duflx_dt(*)
            type(c_ptr), value :: uflxc, dflxc, duflxc_dt, uflx_adj, hr_adj, uflxc_adj, hrc_adj
            integer(c_int) :: rc
         end function rrtmg_lw_hip_adjust_tsfc
         function rrtmg_lw_hip_adjust_tsfc_r4(ncol, nlay, plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt, &
               uflx_adj, hr_adj, uflxc_adj, hrc_adj) bind(C, name='rrtmg_lw_hip_adjust_tsfc_r4') result(rc)
            import :: c_int, c_float, c_ptr
            integer(c_int), value :: ncol, nlay
            real(c_float), intent(in) :: plev(*), dtsfc(*), uflx(*), dflx(*), duflx_dt(*)
            type(c_ptr), value :: uflxc, dflxc, duflxc_dt, uflx_adj, hr_adj, uflxc_adj, hrc_adj
            integer(c_int) :: rc
         end function rrtmg_lw_hip_adjust_tsfc_r4
      end interface

      contains

      subroutine rrtmg_lw_dtsfc_r8 &
            (ncol    ,nlay    ,plev    ,dtsfc   , &
             uflx    ,dflx    ,duflx_dt,uflx_adj,hr_adj  , &
             uflxc   ,dflxc   ,duflxc_dt,uflxc_adj,hrc_adj)

      integer(kind=im), intent(in) :: ncol            ! Number of horizontal columns
      integer(kind=im), intent(in) :: nlay            ! Number of model layers
      real(kind=rb), intent(in) :: plev(:,:)          ! Interface pressures (hPa, mb)                    (ncol,nlay+1)
      real(kind=rb), intent(in) :: dtsfc(:)           ! Surface temperature now minus that of the radiation call (K)   (ncol)
      real(kind=rb), intent(in) :: uflx(:,:)          ! Total sky upward flux of the radiation call (W/m2)         (ncol,nlay+1)
      real(kind=rb), intent(in) :: dflx(:,:)          ! Total sky downward flux (W/m2)
      real(kind=rb), intent(in) :: duflx_dt(:,:)      ! Change of the upward flux with surface temperature (W/m2/K)
      real(kind=rb), intent(out), target :: uflx_adj(:,:)   ! Adjusted total sky upward flux (W/m2)           (ncol,nlay+1)
      real(kind=rb), intent(out), target :: hr_adj(:,:)     ! Adjusted total sky heating rate (K/d)            (ncol,nlay)
      real(kind=rb), intent(in), optional, target :: uflxc(:,:), dflxc(:,:), duflxc_dt(:,:)        ! the same, clear sky
      real(kind=rb), intent(out), optional, target :: uflxc_adj(:,:), hrc_adj(:,:)

      integer(c_int) :: rc, np
      real(c_double), allocatable, target :: t1(:,:), t2(:,:), t3(:,:), t4(:,:), t5(:,:), t6(:,:), t7(:,:)
      type(c_ptr) :: p1, p2, p3, p4, p5, p6, p7

      np = 0
      if (present(uflxc)) np = np + 1
      if (present(dflxc)) np = np + 1
      if (present(duflxc_dt)) np = np + 1
      if (present(uflxc_adj)) np = np + 1
      if (present(hrc_adj)) np = np + 1
      if (np /= 0 .and. np /= 5) then
         write(*,'(a)') 'rrtmg_lw_dtsfc: uflxc, dflxc, duflxc_dt, uflxc_adj and hrc_adj must be all present or all absent'
         error stop 1
      endif
      call check_extent('plev', size(plev,1), size(plev,2), ncol, nlay+1)
      call check_extent('uflx', size(uflx,1), size(uflx,2), ncol, nlay+1)
      call check_extent('dflx', size(dflx,1), size(dflx,2), ncol, nlay+1)
      call check_extent('duflx_dt', size(duflx_dt,1), size(duflx_dt,2), ncol, nlay+1)
      if (size(dtsfc) < ncol) then
         write(*,'(a,i0,a,i0)') 'rrtmg_lw_dtsfc: dtsfc has ', size(dtsfc), ' values, fewer than ', ncol
         error stop 1
      endif
      p1 = c_null_ptr; p2 = c_null_ptr; p3 = c_null_ptr; p6 = c_null_ptr; p7 = c_null_ptr
      call across('uflx_adj', uflx_adj, t4, p4, ncol, nlay+1, .false.)
      call across('hr_adj', hr_adj, t5, p5, ncol, nlay, .false.)
      if (np == 5) then
         call across('uflxc', uflxc, t1, p1, ncol, nlay+1, .true.)
         call across('dflxc', dflxc, t2, p2, ncol, nlay+1, .true.)
         call across('duflxc_dt', duflxc_dt, t3, p3, ncol, nlay+1, .true.)
         call across('uflxc_adj', uflxc_adj, t6, p6, ncol, nlay+1, .false.)
         call across('hrc_adj', hrc_adj, t7, p7, ncol, nlay, .false.)
      endif
      rc = rrtmg_lw_hip_adjust_tsfc(int(ncol, c_int), int(nlay, c_int), plev(1:ncol,1:nlay+1), dtsfc(1:ncol), &
            uflx(1:ncol,1:nlay+1), dflx(1:ncol,1:nlay+1), duflx_dt(1:ncol,1:nlay+1), p1, p2, p3, p4, p5, p6, p7)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_dtsfc')
      if (allocated(t4)) uflx_adj(1:ncol, 1:nlay+1) = t4
      if (allocated(t5)) hr_adj(1:ncol, 1:nlay) = t5
      if (allocated(t6)) uflxc_adj(1:ncol, 1:nlay+1) = t6
      if (allocated(t7)) hrc_adj(1:ncol, 1:nlay) = t7

      end subroutine rrtmg_lw_dtsfc_r8

      ! the real(4) specific: the same body on float arrays
      subroutine rrtmg_lw_dtsfc_r4 &
            (ncol    ,nlay    ,plev    ,dtsfc   , &
             uflx    ,dflx    ,duflx_dt,uflx_adj,hr_adj  , &
             uflxc   ,dflxc   ,duflxc_dt,uflxc_adj,hrc_adj)

      integer(kind=im), intent(in) :: ncol            ! Number of horizontal columns
      integer(kind=im), intent(in) :: nlay            ! Number of model layers
      real(kind=r4), intent(in) :: plev(:,:)          ! Interface pressures (hPa, mb)                    (ncol,nlay+1)
      real(kind=r4), intent(in) :: dtsfc(:)           ! Surface temperature now minus that of the radiation call (K)   (ncol)
      real(kind=r4), intent(in) :: uflx(:,:)          ! Total sky upward flux of the radiation call (W/m2)         (ncol,nlay+1)
      real(kind=r4), intent(in) :: dflx(:,:)          ! Total sky downward flux (W/m2)
      real(kind=r4), intent(in) :: duflx_dt(:,:)      ! Change of the upward flux with surface temperature (W/m2/K)
      real(kind=r4), intent(out), target :: uflx_adj(:,:)   ! Adjusted total sky upward flux (W/m2)           (ncol,nlay+1)
      real(kind=r4), intent(out), target :: hr_adj(:,:)     ! Adjusted total sky heating rate (K/d)            (ncol,nlay)
      real(kind=r4), intent(in), optional, target :: uflxc(:,:), dflxc(:,:), duflxc_dt(:,:)        ! the same, clear sky
      real(kind=r4), intent(out), optional, target :: uflxc_adj(:,:), hrc_adj(:,:)

      integer(c_int) :: rc, np
      real(c_float), allocatable, target :: t1(:,:), t2(:,:), t3(:,:), t4(:,:), t5(:,:), t6(:,:), t7(:,:)
      type(c_ptr) :: p1, p2, p3, p4, p5, p6, p7

      np = 0
      if (present(uflxc)) np = np + 1
      if (present(dflxc)) np = np + 1
      if (present(duflxc_dt)) np = np + 1
      if (present(uflxc_adj)) np = np + 1
      if (present(hrc_adj)) np = np + 1
      if (np /= 0 .and. np /= 5) then
         write(*,'(a)') 'rrtmg_lw_dtsfc: uflxc, dflxc, duflxc_dt, uflxc_adj and hrc_adj must be all present or all absent'
         error stop 1
      endif
      call check_extent('plev', size(plev,1), size(plev,2), ncol, nlay+1)
      call check_extent('uflx', size(uflx,1), size(uflx,2), ncol, nlay+1)
      call check_extent('dflx', size(dflx,1), size(dflx,2), ncol, nlay+1)
      call check_extent('duflx_dt', size(duflx_dt,1), size(duflx_dt,2), ncol, nlay+1)
      if (size(dtsfc) < ncol) then
         write(*,'(a,i0,a,i0)') 'rrtmg_lw_dtsfc: dtsfc has ', size(dtsfc), ' values, fewer than ', ncol
         error stop 1
      endif
      p1 = c_null_ptr; p2 = c_null_ptr; p3 = c_null_ptr; p6 = c_null_ptr; p7 = c_null_ptr
      call across_r4('uflx_adj', uflx_adj, t4, p4, ncol, nlay+1, .false.)
      call across_r4('hr_adj', hr_adj, t5, p5, ncol, nlay, .false.)
      if (np == 5) then
         call across_r4('uflxc', uflxc, t1, p1, ncol, nlay+1, .true.)
         call across_r4('dflxc', dflxc, t2, p2, ncol, nlay+1, .true.)
         call across_r4('duflxc_dt', duflxc_dt, t3, p3, ncol, nlay+1, .true.)
         call across_r4('uflxc_adj', uflxc_adj, t6, p6, ncol, nlay+1, .false.)
         call across_r4('hrc_adj', hrc_adj, t7, p7, ncol, nlay, .false.)
      endif
      rc = rrtmg_lw_hip_adjust_tsfc_r4(int(ncol, c_int), int(nlay, c_int), plev(1:ncol,1:nlay+1), dtsfc(1:ncol), &
            uflx(1:ncol,1:nlay+1), dflx(1:ncol,1:nlay+1), duflx_dt(1:ncol,1:nlay+1), p1, p2, p3, p4, p5, p6, p7)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_dtsfc')
      if (allocated(t4)) uflx_adj(1:ncol, 1:nlay+1) = t4
      if (allocated(t5)) hr_adj(1:ncol, 1:nlay) = t5
      if (allocated(t6)) uflxc_adj(1:ncol, 1:nlay+1) = t6
      if (allocated(t7)) hrc_adj(1:ncol, 1:nlay) = t7

      end subroutine rrtmg_lw_dtsfc_r4

      ! an optional input or an output (n1,n2) as a C pointer: exactly sized, contiguous actuals go across in place; larger or strided
      ! ones through the temporary t - filled from the section for an input, copied back by the caller for an output
      subroutine across(name, a, t, p, n1, n2, input)
      character(len=*), intent(in) :: name
      real(kind=rb), target :: a(:,:)                  ! (no intent: an input of the caller, or an output the library fills through p)
      real(c_double), allocatable, target, intent(inout) :: t(:,:)
      type(c_ptr), intent(out) :: p
      integer(kind=im), intent(in) :: n1, n2
      logical, intent(in) :: input
      call check_extent(name, size(a,1), size(a,2), n1, n2)
      if (size(a,1) == n1 .and. size(a,2) == n2 .and. is_contiguous(a)) then
         p = c_loc(a)
      else
         allocate(t(n1, n2))
         if (input) t = a(1:n1, 1:n2)
         p = c_loc(t)
      endif
      end subroutine across

      subroutine across_r4(name, a, t, p, n1, n2, input)
      character(len=*), intent(in) :: name
      real(kind=r4), target :: a(:,:)                  ! (no intent: an input of the caller, or an output the library fills through p)
      real(c_float), allocatable, target, intent(inout) :: t(:,:)
      type(c_ptr), intent(out) :: p
      integer(kind=im), intent(in) :: n1, n2
      logical, intent(in) :: input
      call check_extent(name, size(a,1), size(a,2), n1, n2)
      if (size(a,1) == n1 .and. size(a,2) == n2 .and. is_contiguous(a)) then
         p = c_loc(a)
      else
         allocate(t(n1, n2))
         if (input) t = a(1:n1, 1:n2)
         p = c_loc(t)
      endif
      end subroutine across_r4

      subroutine check_extent(name, n1, n2, ncol, nl)
      character(len=*), intent(in) :: name
      integer, intent(in) :: n1, n2
      integer(kind=im), intent(in) :: ncol, nl
      if (n1 < ncol .or. n2 < nl) then
         write(*,'(a,a,a,i0,a,i0,a,i0,a,i0,a)') 'rrtmg_lw_dtsfc: ', name, ' has extents (', n1, ',', n2, &
               '), smaller than (', ncol, ',', nl, ')'
         error stop 1
      endif
      end subroutine check_extent

      end module rrtmg_lw_adjust
