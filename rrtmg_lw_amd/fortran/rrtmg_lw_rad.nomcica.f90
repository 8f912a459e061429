!  Drop-in replacement for the reference's module rrtmg_lw_rad, non-McICA flavour
!  (src/rrtmg_lw_rad.nomcica.f90:99-108): same module name, subroutine name, argument order, kinds,
!  intents and assumed-shape dummies, so a host model's
!      use rrtmg_lw_rad, only: rrtmg_lw
!      call rrtmg_lw(ncol, nlay, icld, idrv, play, plev, ..., uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt)
!  compiles unchanged.  The body forwards to rrtmg_lw_hip_run_nomcica (include/rrtmg_lw_hip.h) the sections
!  (1:ncol, 1:nlay[+1]) of its arguments - what the reference's loops touch - so oversized (pcols > ncol) and
!  strided actuals behave as with the reference.
      module rrtmg_lw_rad

      use iso_c_binding
      use parkind, only : im => kind_im, rb => kind_rb
      use rrtmg_lw_init, only : rrtmg_lw_hip_abort

      implicit none

      public :: rrtmg_lw

!  rrtmg_lw is generic over the real kind: the reference's real(kind_rb) and real(4), for a host built with 4-byte reals (no -r8).  The
!  real(4) specific forwards to rrtmg_lw_hip_run_nomcica_r4 (include/rrtmg_lw_hip.h, "_r4"): the arrays cross as float32, the solver works
!  in float64 on the widened values and the results are rounded.  The same rules: sections (1:ncol, 1:nlay[+1]), exactly sized contiguous
!  duflx_dt / duflxc_dt in place, extent checks.  The spectral optionals are on the real(kind_rb) specific only.
      integer, parameter, private :: r4 = c_float

      interface rrtmg_lw
         module procedure rrtmg_lw_r8, rrtmg_lw_r4
      end interface

      interface
         function rrtmg_lw_hip_run_nomcica(ncol, nlay, icld, idrv, play, plev, tlay, tlev, tsfc, &
               h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
               inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt) bind(C, name='rrtmg_lw_hip_run_nomcica') result(rc)
            import :: c_int, c_double, c_ptr
            integer(c_int), value :: ncol, nlay, idrv, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld
            real(c_double), intent(in) :: play(*), plev(*), tlay(*), tlev(*), tsfc(*), h2ovmr(*), o3vmr(*), co2vmr(*)
            real(c_double), intent(in) :: ch4vmr(*), n2ovmr(*), o2vmr(*), cfc11vmr(*), cfc12vmr(*), cfc22vmr(*), ccl4vmr(*)
            real(c_double), intent(in) :: emis(*), cldfr(*), taucld(*), cicewp(*), cliqwp(*), reice(*), reliq(*), tauaer(*)
            real(c_double), intent(out) :: uflx(*), dflx(*), hr(*), uflxc(*), dflxc(*), hrc(*)
            type(c_ptr), value :: duflx_dt, duflxc_dt
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_nomcica
         function rrtmg_lw_hip_run_nomcica_r4(ncol, nlay, icld, idrv, play, plev, tlay, tlev, tsfc, &
               h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
               inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt) bind(C, name='rrtmg_lw_hip_run_nomcica_r4') result(rc)
            import :: c_int, c_float, c_ptr
            integer(c_int), value :: ncol, nlay, idrv, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld
            real(c_float), intent(in) :: play(*), plev(*), tlay(*), tlev(*), tsfc(*), h2ovmr(*), o3vmr(*), co2vmr(*)
            real(c_float), intent(in) :: ch4vmr(*), n2ovmr(*), o2vmr(*), cfc11vmr(*), cfc12vmr(*), cfc22vmr(*), ccl4vmr(*)
            real(c_float), intent(in) :: emis(*), cldfr(*), taucld(*), cicewp(*), cliqwp(*), reice(*), reliq(*), tauaer(*)
            real(c_float), intent(out) :: uflx(*), dflx(*), hr(*), uflxc(*), dflxc(*), hrc(*)
            type(c_ptr), value :: duflx_dt, duflxc_dt
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_nomcica_r4
         function rrtmg_lw_hip_run_nomcica_spectral(ncol, nlay, icld, idrv, play, plev, tlay, tlev, tsfc, &
               h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
               inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, &
               uflxs, dflxs, uflxcs, dflxcs) bind(C, name='rrtmg_lw_hip_run_nomcica_spectral') result(rc)
            import :: c_int, c_double, c_ptr
            integer(c_int), value :: ncol, nlay, idrv, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld
            real(c_double), intent(in) :: play(*), plev(*), tlay(*), tlev(*), tsfc(*), h2ovmr(*), o3vmr(*), co2vmr(*)
            real(c_double), intent(in) :: ch4vmr(*), n2ovmr(*), o2vmr(*), cfc11vmr(*), cfc12vmr(*), cfc22vmr(*), ccl4vmr(*)
            real(c_double), intent(in) :: emis(*), cldfr(*), taucld(*), cicewp(*), cliqwp(*), reice(*), reliq(*), tauaer(*)
            real(c_double), intent(out) :: uflx(*), dflx(*), hr(*), uflxc(*), dflxc(*), hrc(*)
            type(c_ptr), value :: duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_nomcica_spectral
      end interface

      contains

      subroutine rrtmg_lw_r8 &
            (ncol    ,nlay    ,icld    ,idrv    , &
             play    ,plev    ,tlay    ,tlev    ,tsfc    , &
             h2ovmr  ,o3vmr   ,co2vmr  ,ch4vmr  ,n2ovmr  ,o2vmr , &
             cfc11vmr,cfc12vmr,cfc22vmr,ccl4vmr ,emis    , &
             inflglw ,iceflglw,liqflglw,cldfr   , &
             taucld  ,cicewp  ,cliqwp  ,reice   ,reliq   , &
             tauaer  , &
             uflx    ,dflx    ,hr      ,uflxc   ,dflxc,  hrc, &
             duflx_dt,duflxc_dt, &
             uflxs   ,dflxs   ,uflxcs  ,dflxcs )

      integer(kind=im), intent(in) :: ncol            ! Number of horizontal columns
      integer(kind=im), intent(in) :: nlay            ! Number of model layers
      integer(kind=im), intent(inout) :: icld         ! Cloud overlap method
      integer(kind=im), intent(in) :: idrv            ! Flag for calculation of dFdT
      real(kind=rb), intent(in) :: play(:,:)          ! Layer pressures (hPa, mb)           (ncol,nlay)
      real(kind=rb), intent(in) :: plev(:,:)          ! Interface pressures (hPa, mb)       (ncol,nlay+1)
      real(kind=rb), intent(in) :: tlay(:,:)          ! Layer temperatures (K)
      real(kind=rb), intent(in) :: tlev(:,:)          ! Interface temperatures (K)
      real(kind=rb), intent(in) :: tsfc(:)            ! Surface temperature (K)
      real(kind=rb), intent(in) :: h2ovmr(:,:), o3vmr(:,:), co2vmr(:,:), ch4vmr(:,:), n2ovmr(:,:), o2vmr(:,:)
      real(kind=rb), intent(in) :: cfc11vmr(:,:), cfc12vmr(:,:), cfc22vmr(:,:), ccl4vmr(:,:)
      real(kind=rb), intent(in) :: emis(:,:)          ! Surface emissivity                  (ncol,nbndlw)
      integer(kind=im), intent(in) :: inflglw, iceflglw, liqflglw
      real(kind=rb), intent(in) :: cldfr(:,:)         ! Cloud fraction                      (ncol,nlay)
      real(kind=rb), intent(in) :: cicewp(:,:), cliqwp(:,:), reice(:,:), reliq(:,:)
      real(kind=rb), intent(in) :: taucld(:,:,:)      ! In-cloud optical depth              (nbndlw,ncol,nlay)
      real(kind=rb), intent(in) :: tauaer(:,:,:)      ! Aerosol optical depth               (ncol,nlay,nbndlw)
      real(kind=rb), intent(out) :: uflx(:,:), dflx(:,:), hr(:,:), uflxc(:,:), dflxc(:,:), hrc(:,:)
      real(kind=rb), intent(out), optional, target :: duflx_dt(:,:), duflxc_dt(:,:)
      ! Spectral outputs (optional, this library's extension; include/rrtmg_lw_hip.h, "Spectral (per-band) fluxes"):
      ! per band the flux the band adds to uflx / dflx / uflxc / dflxc, (ncol,nlay+1,nbndlw), band 16 in the broadband
      ! call's convention (2600 cm-1 to infinity).  uflxs and dflxs together; uflxcs and dflxcs together, or neither.
      ! Absent: the plain call.
      real(kind=rb), intent(out), optional, target :: uflxs(:,:,:), dflxs(:,:,:), uflxcs(:,:,:), dflxcs(:,:,:)

      integer(c_int) :: rc, icld_c
      real(c_double), allocatable, target :: d1(:,:), d2(:,:)
      type(c_ptr) :: p1, p2
      logical :: inplace
      real(c_double), allocatable, target :: s1(:,:,:), s2(:,:,:), s3(:,:,:), s4(:,:,:)
      type(c_ptr) :: q1, q2, q3, q4
      logical :: spectral

      icld_c = int(icld, c_int)
      p1 = c_null_ptr
      p2 = c_null_ptr
      inplace = .false.
      if (idrv == 1) then
         if (.not. (present(duflx_dt) .and. present(duflxc_dt))) then
            write(*,*) 'rrtmg_lw: idrv = 1 requires duflx_dt and duflxc_dt'
            error stop 1
         endif
         ! exactly sized, contiguous actuals go across in place like every other array (and stay page-locked if the host pinned them:
         ! rrtmg_lw_pin); an optional dummy cannot be passed as a section, so anything else goes through a temporary
         inplace = size(duflx_dt,1) == ncol .and. size(duflx_dt,2) == nlay+1 .and. is_contiguous(duflx_dt) .and. &
                   size(duflxc_dt,1) == ncol .and. size(duflxc_dt,2) == nlay+1 .and. is_contiguous(duflxc_dt)
         if (inplace) then
            p1 = c_loc(duflx_dt)
            p2 = c_loc(duflxc_dt)
         else
            if (size(duflx_dt,1) < ncol .or. size(duflx_dt,2) < nlay+1 .or. size(duflxc_dt,1) < ncol .or. size(duflxc_dt,2) < nlay+1) then
               write(*,*) 'rrtmg_lw: duflx_dt / duflxc_dt smaller than (ncol, nlay+1)'
               error stop 1
            endif
            allocate(d1(ncol, nlay+1), d2(ncol, nlay+1))
            p1 = c_loc(d1)
            p2 = c_loc(d2)
         endif
      endif
      ! The reference indexes play(iplon,lay) etc. (src/rrtmg_lw_rad.nomcica.f90:785-910), so a host may pass arrays that are
      ! larger than (ncol,nlay) - e.g. dimensioned (pcols,pver) with ncol < pcols - or strided sections.  The C side strides by
      ! exactly ncol: every array goes across as the section the reference would touch (the compiler packs / unpacks when that
      ! section is not contiguous; exactly-sized contiguous arrays are passed in place).
      call check_extent('play', size(play,1), size(play,2), ncol, nlay)
      call check_extent('plev', size(plev,1), size(plev,2), ncol, nlay+1)
      call check_extent('tauaer', size(tauaer,1), size(tauaer,2), ncol, nlay)
      call check_extent('taucld', size(taucld,2), size(taucld,3), ncol, nlay)
      call check_extent('uflx', size(uflx,1), size(uflx,2), ncol, nlay+1)
      call check_extent('hr', size(hr,1), size(hr,2), ncol, nlay)
      spectral = present(uflxs) .or. present(dflxs) .or. present(uflxcs) .or. present(dflxcs)
      q3 = c_null_ptr
      q4 = c_null_ptr
      if (spectral) then
         if (.not. (present(uflxs) .and. present(dflxs))) then
            write(*,*) 'rrtmg_lw: spectral outputs need uflxs and dflxs'
            error stop 1
         endif
         if (present(uflxcs) .neqv. present(dflxcs)) then
            write(*,*) 'rrtmg_lw: uflxcs and dflxcs go together'
            error stop 1
         endif
         call spec_arg('uflxs', uflxs, s1, q1, ncol, nlay)
         call spec_arg('dflxs', dflxs, s2, q2, ncol, nlay)
         if (present(uflxcs)) then
            call spec_arg('uflxcs', uflxcs, s3, q3, ncol, nlay)
            call spec_arg('dflxcs', dflxcs, s4, q4, ncol, nlay)
         endif
      endif
      if (spectral) then
         rc = rrtmg_lw_hip_run_nomcica_spectral(int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), &
               play(1:ncol,1:nlay), plev(1:ncol,1:nlay+1), tlay(1:ncol,1:nlay), tlev(1:ncol,1:nlay+1), tsfc(1:ncol), &
               h2ovmr(1:ncol,1:nlay), o3vmr(1:ncol,1:nlay), co2vmr(1:ncol,1:nlay), ch4vmr(1:ncol,1:nlay), &
               n2ovmr(1:ncol,1:nlay), o2vmr(1:ncol,1:nlay), cfc11vmr(1:ncol,1:nlay), cfc12vmr(1:ncol,1:nlay), &
               cfc22vmr(1:ncol,1:nlay), ccl4vmr(1:ncol,1:nlay), emis(1:ncol,1:16), &
               int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), &
               cldfr(1:ncol,1:nlay), taucld(1:16,1:ncol,1:nlay), cicewp(1:ncol,1:nlay), cliqwp(1:ncol,1:nlay), &
               reice(1:ncol,1:nlay), reliq(1:ncol,1:nlay), tauaer(1:ncol,1:nlay,1:16), &
               uflx(1:ncol,1:nlay+1), dflx(1:ncol,1:nlay+1), hr(1:ncol,1:nlay), &
               uflxc(1:ncol,1:nlay+1), dflxc(1:ncol,1:nlay+1), hrc(1:ncol,1:nlay), p1, p2, q1, q2, q3, q4)
      else
         rc = rrtmg_lw_hip_run_nomcica(int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), &
               play(1:ncol,1:nlay), plev(1:ncol,1:nlay+1), tlay(1:ncol,1:nlay), tlev(1:ncol,1:nlay+1), tsfc(1:ncol), &
               h2ovmr(1:ncol,1:nlay), o3vmr(1:ncol,1:nlay), co2vmr(1:ncol,1:nlay), ch4vmr(1:ncol,1:nlay), &
               n2ovmr(1:ncol,1:nlay), o2vmr(1:ncol,1:nlay), cfc11vmr(1:ncol,1:nlay), cfc12vmr(1:ncol,1:nlay), &
               cfc22vmr(1:ncol,1:nlay), ccl4vmr(1:ncol,1:nlay), emis(1:ncol,1:16), &
               int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), &
               cldfr(1:ncol,1:nlay), taucld(1:16,1:ncol,1:nlay), cicewp(1:ncol,1:nlay), cliqwp(1:ncol,1:nlay), &
               reice(1:ncol,1:nlay), reliq(1:ncol,1:nlay), tauaer(1:ncol,1:nlay,1:16), &
               uflx(1:ncol,1:nlay+1), dflx(1:ncol,1:nlay+1), hr(1:ncol,1:nlay), &
               uflxc(1:ncol,1:nlay+1), dflxc(1:ncol,1:nlay+1), hrc(1:ncol,1:nlay), p1, p2)
      endif
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw')
      icld = int(icld_c, im)
      if (idrv == 1 .and. .not. inplace) then
         duflx_dt(1:ncol, 1:nlay+1) = d1
         duflxc_dt(1:ncol, 1:nlay+1) = d2
      endif

      if (allocated(s1)) uflxs(1:ncol, 1:nlay+1, 1:16) = s1
      if (allocated(s2)) dflxs(1:ncol, 1:nlay+1, 1:16) = s2
      if (allocated(s3)) uflxcs(1:ncol, 1:nlay+1, 1:16) = s3
      if (allocated(s4)) dflxcs(1:ncol, 1:nlay+1, 1:16) = s4

      end subroutine rrtmg_lw_r8

      ! the real(4) specific: the same body on float arrays, without the spectral optionals
      subroutine rrtmg_lw_r4 &
            (ncol    ,nlay    ,icld    ,idrv    , &
             play    ,plev    ,tlay    ,tlev    ,tsfc    , &
             h2ovmr  ,o3vmr   ,co2vmr  ,ch4vmr  ,n2ovmr  ,o2vmr , &
             cfc11vmr,cfc12vmr,cfc22vmr,ccl4vmr ,emis    , &
             inflglw ,iceflglw,liqflglw,cldfr   , &
             taucld  ,cicewp  ,cliqwp  ,reice   ,reliq   , &
             tauaer  , &
             uflx    ,dflx    ,hr      ,uflxc   ,dflxc,  hrc, &
             duflx_dt,duflxc_dt)

      integer(kind=im), intent(in) :: ncol            ! Number of horizontal columns
      integer(kind=im), intent(in) :: nlay            ! Number of model layers
      integer(kind=im), intent(inout) :: icld         ! Cloud overlap method
      integer(kind=im), intent(in) :: idrv            ! Flag for calculation of dFdT
      real(kind=r4), intent(in) :: play(:,:)          ! Layer pressures (hPa, mb)           (ncol,nlay)
      real(kind=r4), intent(in) :: plev(:,:)          ! Interface pressures (hPa, mb)       (ncol,nlay+1)
      real(kind=r4), intent(in) :: tlay(:,:)          ! Layer temperatures (K)
      real(kind=r4), intent(in) :: tlev(:,:)          ! Interface temperatures (K)
      real(kind=r4), intent(in) :: tsfc(:)            ! Surface temperature (K)
      real(kind=r4), intent(in) :: h2ovmr(:,:), o3vmr(:,:), co2vmr(:,:), ch4vmr(:,:), n2ovmr(:,:), o2vmr(:,:)
      real(kind=r4), intent(in) :: cfc11vmr(:,:), cfc12vmr(:,:), cfc22vmr(:,:), ccl4vmr(:,:)
      real(kind=r4), intent(in) :: emis(:,:)          ! Surface emissivity                  (ncol,nbndlw)
      integer(kind=im), intent(in) :: inflglw, iceflglw, liqflglw
      real(kind=r4), intent(in) :: cldfr(:,:)         ! Cloud fraction                      (ncol,nlay)
      real(kind=r4), intent(in) :: cicewp(:,:), cliqwp(:,:), reice(:,:), reliq(:,:)
      real(kind=r4), intent(in) :: taucld(:,:,:)      ! In-cloud optical depth              (nbndlw,ncol,nlay)
      real(kind=r4), intent(in) :: tauaer(:,:,:)      ! Aerosol optical depth               (ncol,nlay,nbndlw)
      real(kind=r4), intent(out) :: uflx(:,:), dflx(:,:), hr(:,:), uflxc(:,:), dflxc(:,:), hrc(:,:)
      real(kind=r4), intent(out), optional, target :: duflx_dt(:,:), duflxc_dt(:,:)

      integer(c_int) :: rc, icld_c
      real(c_float), allocatable, target :: d1(:,:), d2(:,:)
      type(c_ptr) :: p1, p2
      logical :: inplace

      icld_c = int(icld, c_int)
      p1 = c_null_ptr
      p2 = c_null_ptr
      inplace = .false.
      if (idrv == 1) then
         if (.not. (present(duflx_dt) .and. present(duflxc_dt))) then
            write(*,*) 'rrtmg_lw: idrv = 1 requires duflx_dt and duflxc_dt'
            error stop 1
         endif
         ! exactly sized, contiguous actuals go across in place like every other array (and stay page-locked if the host pinned them:
         ! rrtmg_lw_pin); an optional dummy cannot be passed as a section, so anything else goes through a temporary
         inplace = size(duflx_dt,1) == ncol .and. size(duflx_dt,2) == nlay+1 .and. is_contiguous(duflx_dt) .and. &
                   size(duflxc_dt,1) == ncol .and. size(duflxc_dt,2) == nlay+1 .and. is_contiguous(duflxc_dt)
         if (inplace) then
            p1 = c_loc(duflx_dt)
            p2 = c_loc(duflxc_dt)
         else
            if (size(duflx_dt,1) < ncol .or. size(duflx_dt,2) < nlay+1 .or. size(duflxc_dt,1) < ncol .or. size(duflxc_dt,2) < nlay+1) then
               write(*,*) 'rrtmg_lw: duflx_dt / duflxc_dt smaller than (ncol, nlay+1)'
               error stop 1
            endif
            allocate(d1(ncol, nlay+1), d2(ncol, nlay+1))
            p1 = c_loc(d1)
            p2 = c_loc(d2)
         endif
      endif
      ! The reference indexes play(iplon,lay) etc. (src/rrtmg_lw_rad.nomcica.f90:785-910), so a host may pass arrays that are
      ! larger than (ncol,nlay) - e.g. dimensioned (pcols,pver) with ncol < pcols - or strided sections.  The C side strides by
      ! exactly ncol: every array goes across as the section the reference would touch (the compiler packs / unpacks when that
      ! section is not contiguous; exactly-sized contiguous arrays are passed in place).
      call check_extent('play', size(play,1), size(play,2), ncol, nlay)
      call check_extent('plev', size(plev,1), size(plev,2), ncol, nlay+1)
      call check_extent('tauaer', size(tauaer,1), size(tauaer,2), ncol, nlay)
      call check_extent('taucld', size(taucld,2), size(taucld,3), ncol, nlay)
      call check_extent('uflx', size(uflx,1), size(uflx,2), ncol, nlay+1)
      call check_extent('hr', size(hr,1), size(hr,2), ncol, nlay)
      rc = rrtmg_lw_hip_run_nomcica_r4(int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), &
            play(1:ncol,1:nlay), plev(1:ncol,1:nlay+1), tlay(1:ncol,1:nlay), tlev(1:ncol,1:nlay+1), tsfc(1:ncol), &
            h2ovmr(1:ncol,1:nlay), o3vmr(1:ncol,1:nlay), co2vmr(1:ncol,1:nlay), ch4vmr(1:ncol,1:nlay), &
            n2ovmr(1:ncol,1:nlay), o2vmr(1:ncol,1:nlay), cfc11vmr(1:ncol,1:nlay), cfc12vmr(1:ncol,1:nlay), &
            cfc22vmr(1:ncol,1:nlay), ccl4vmr(1:ncol,1:nlay), emis(1:ncol,1:16), &
            int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), &
            cldfr(1:ncol,1:nlay), taucld(1:16,1:ncol,1:nlay), cicewp(1:ncol,1:nlay), cliqwp(1:ncol,1:nlay), &
            reice(1:ncol,1:nlay), reliq(1:ncol,1:nlay), tauaer(1:ncol,1:nlay,1:16), &
            uflx(1:ncol,1:nlay+1), dflx(1:ncol,1:nlay+1), hr(1:ncol,1:nlay), &
            uflxc(1:ncol,1:nlay+1), dflxc(1:ncol,1:nlay+1), hrc(1:ncol,1:nlay), p1, p2)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw')
      icld = int(icld_c, im)
      if (idrv == 1 .and. .not. inplace) then
         duflx_dt(1:ncol, 1:nlay+1) = d1
         duflxc_dt(1:ncol, 1:nlay+1) = d2
      endif

      end subroutine rrtmg_lw_r4

      ! a spectral output (ncol,nlay+1,16): exactly sized, contiguous actuals go across in place (like duflx_dt);
      ! larger or strided ones through the temporary t, copied back after the call
      subroutine spec_arg(name, a, t, p, ncol, nlay)
      character(len=*), intent(in) :: name
      real(kind=rb), intent(inout), target :: a(:,:,:)
      real(c_double), allocatable, target, intent(inout) :: t(:,:,:)
      type(c_ptr), intent(out) :: p
      integer(kind=im), intent(in) :: ncol, nlay
      if (size(a,1) < ncol .or. size(a,2) < nlay+1 .or. size(a,3) < 16) then
         write(*,'(a,a,a)') 'rrtmg_lw: ', name, ' smaller than (ncol, nlay+1, 16)'
         error stop 1
      endif
      if (size(a,1) == ncol .and. size(a,2) == nlay+1 .and. size(a,3) == 16 .and. is_contiguous(a)) then
         p = c_loc(a)
      else
         allocate(t(ncol, nlay+1, 16))
         p = c_loc(t)
      endif
      end subroutine spec_arg

      subroutine check_extent(name, n1, n2, ncol, nl)
      character(len=*), intent(in) :: name
      integer, intent(in) :: n1, n2
      integer(kind=im), intent(in) :: ncol, nl
      if (n1 < ncol .or. n2 < nl) then
         write(*,'(a,a,a,i0,a,i0,a,i0,a,i0,a)') 'rrtmg_lw: ', name, ' has extents (', n1, ',', n2, &
               '), smaller than (', ncol, ',', nl, ')'
         error stop 1
      endif
      end subroutine check_extent

      end module rrtmg_lw_rad
