!  Gas optics and Planck sources of rrtmg_lw (this library's extension; include/rrtmg_lw_hip.h, "Gas optics and Planck sources"):
!      use rrtmg_lw_optics, only: rrtmg_lw_gas_optics
!      call rrtmg_lw_gas_optics(ncol, nlay, play, plev, tlay, tlev, tsfc, h2ovmr, ..., ccl4vmr, emis, taug, fracs &
!                               [, planklay, planklev, plankbnd, dplankbnd_dt])
!  The GCM inputs of rrtmg_lw (module rrtmg_lw_rad) without the cloud and aerosol arrays.  Outputs:
!      taug, fracs    (ncol,nlay,ngptlw)  taumol's gas optical depth (no aerosol, no diffusivity secant) and Planck fraction per g-point
!      planklay       (ncol,nlay,nbndlw)  setcoef's Planck integrals of the layers;  planklev (ncol,0:nlay,nbndlw) of the levels
!      plankbnd       (ncol,nbndlw)       surface Planck integrals times emis;  dplankbnd_dt (ncol,nbndlw) their d/dT
!  ngptlw = rrtmg_lw_hip_gpoints() (140, or 256 with librrtmg_lw_hip_g256.so).  The Planck outputs are optional; an absent one is not
!  formed.  dplankbnd_dt present = idrv 1.  Arrays larger than the declared shapes (pcols > ncol) or strided sections are accepted as
!  in rrtmg_lw_rad: the inputs go across as the section (1:ncol, ...), the outputs through temporaries where they are not exactly sized.
!
!  Cloud optics (include/rrtmg_lw_hip.h, "Cloud optics: band optical depths, ncbands, secdiff"):
!      use rrtmg_lw_optics, only: rrtmg_lw_cloud_optics
!      call rrtmg_lw_cloud_optics(ncol, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq &
!                                 [, plev, h2ovmr] [, taucloud] [, ncbands] [, secdiff])
!  The cloud inputs of rrtmg_lw (taucld (nbndlw,ncol,nlay)); imca = 0: cldprop, 1: cldprmc on a cloudy sub-column.  Outputs, each optional,
!  at least one present (pass them by keyword):
!      taucloud       (ncol,nlay,nbndlw)  cloud optical depth per spectral band, before the diffusivity secant
!      ncbands        (ncol)              cldprop's band count at the end of the column (16 with imca = 1)
!      secdiff        (ncol,nbndlw)       the diffusivity secants; needs plev (ncol,nlay+1) and h2ovmr (ncol,nlay)
!  Larger arrays (pcols > ncol) as above.  A particle size out of bounds ends the program with the reference's text (rrtmg_lw_hip_abort).
!
!  The solver on the caller's optical depths and sources (include/rrtmg_lw_hip.h, "The solver on the caller's optical depths and sources"):
!      use rrtmg_lw_optics, only: rrtmg_lw_solve
!      call rrtmg_lw_solve(ncol, nlay, cloud, plev, emis, tau, fracs, planklay, planklev, plankbnd, uflx, dflx, hr &
!                          [, uflxc, dflxc, hrc] [, dplankbnd_dt, duflx_dt, duflxc_dt] [, cldfr] [, odcld] [, submask])
!  tau, fracs (ncol,nlay,ngptlw); planklay, odcld (ncol,nlay,nbndlw); planklev (ncol,0:nlay,nbndlw); emis, plankbnd, dplankbnd_dt
!  (ncol,nbndlw); cldfr (ncol,nlay); submask (ncol,nlay,(ngptlw+31)/32) default-kind C integers as rrtmg_lw_cloud_cover returns them.
!  cloud = 0: no cloud; 1: rtrn on cldfr and odcld; 2: rtrnmc on submask and odcld.  duflx_dt present = idrv 1 (then dplankbnd_dt and
!  duflxc_dt as well).  A host entry: larger arrays (pcols > ncol) as above, nothing outside (1:ncol, ...) is written.
      module rrtmg_lw_optics

      use iso_c_binding
      use parkind, only : im => kind_im, rb => kind_rb
      use rrtmg_lw_init, only : rrtmg_lw_hip_abort

      implicit none

      public :: rrtmg_lw_gas_optics, rrtmg_lw_cloud_optics, rrtmg_lw_solve

      interface
         function rrtmg_lw_hip_solve(ncol, nlay, cloud, idrv, plev, emis, tau, fracs, planklay, planklev, plankbnd, dplankbnd_dt, &
               cldfr, odcld, submask, uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt) bind(C, name='rrtmg_lw_hip_solve') result(rc)
            import :: c_int, c_double, c_ptr
            integer(c_int), value :: ncol, nlay, cloud, idrv
            real(c_double), intent(in) :: plev(*), emis(*), tau(*), fracs(*), planklay(*), planklev(*), plankbnd(*)
            type(c_ptr), value :: dplankbnd_dt, cldfr, odcld, submask, uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt
            integer(c_int) :: rc
         end function rrtmg_lw_hip_solve
         function rrtmg_lw_hip_cloud_optics(ncol, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
               plev, h2ovmr, taucloud, ncbands, secdiff) bind(C, name='rrtmg_lw_hip_cloud_optics') result(rc)
            import :: c_int, c_double, c_ptr
            integer(c_int), value :: ncol, nlay, imca, inflglw, iceflglw, liqflglw
            real(c_double), intent(in) :: cldfr(*), taucld(*), cicewp(*), cliqwp(*), reice(*), reliq(*)
            type(c_ptr), value :: plev, h2ovmr, taucloud, ncbands, secdiff
            integer(c_int) :: rc
         end function rrtmg_lw_hip_cloud_optics
         function rrtmg_lw_hip_gas_optics(ncol, nlay, idrv, play, plev, tlay, tlev, tsfc, &
               h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
               taug, fracs, planklay, planklev, plankbnd, dplankbnd_dt) bind(C, name='rrtmg_lw_hip_gas_optics') result(rc)
            import :: c_int, c_double, c_ptr
            integer(c_int), value :: ncol, nlay, idrv
            real(c_double), intent(in) :: play(*), plev(*), tlay(*), tlev(*), tsfc(*), h2ovmr(*), o3vmr(*), co2vmr(*)
            real(c_double), intent(in) :: ch4vmr(*), n2ovmr(*), o2vmr(*), cfc11vmr(*), cfc12vmr(*), cfc22vmr(*), ccl4vmr(*)
            real(c_double), intent(in) :: emis(*)
            type(c_ptr), value :: taug, fracs, planklay, planklev, plankbnd, dplankbnd_dt
            integer(c_int) :: rc
         end function rrtmg_lw_hip_gas_optics
         function rrtmg_lw_hip_gpoints() bind(C, name='rrtmg_lw_hip_gpoints') result(n)
            import :: c_int
            integer(c_int) :: n
         end function rrtmg_lw_hip_gpoints
      end interface

      contains

      subroutine rrtmg_lw_gas_optics &
            (ncol    ,nlay    , &
             play    ,plev    ,tlay    ,tlev    ,tsfc    , &
             h2ovmr  ,o3vmr   ,co2vmr  ,ch4vmr  ,n2ovmr  ,o2vmr , &
             cfc11vmr,cfc12vmr,cfc22vmr,ccl4vmr ,emis    , &
             taug    ,fracs   , &
             planklay,planklev,plankbnd,dplankbnd_dt)

      integer(kind=im), intent(in) :: ncol            ! Number of horizontal columns
      integer(kind=im), intent(in) :: nlay            ! Number of model layers
      real(kind=rb), intent(in) :: play(:,:)          ! Layer pressures (hPa, mb)           (ncol,nlay)
      real(kind=rb), intent(in) :: plev(:,:)          ! Interface pressures (hPa, mb)       (ncol,nlay+1)
      real(kind=rb), intent(in) :: tlay(:,:)          ! Layer temperatures (K)
      real(kind=rb), intent(in) :: tlev(:,:)          ! Interface temperatures (K)
      real(kind=rb), intent(in) :: tsfc(:)            ! Surface temperature (K)
      real(kind=rb), intent(in) :: h2ovmr(:,:), o3vmr(:,:), co2vmr(:,:), ch4vmr(:,:), n2ovmr(:,:), o2vmr(:,:)
      real(kind=rb), intent(in) :: cfc11vmr(:,:), cfc12vmr(:,:), cfc22vmr(:,:), ccl4vmr(:,:)
      real(kind=rb), intent(in) :: emis(:,:)          ! Surface emissivity                  (ncol,nbndlw)
      real(kind=rb), intent(out), target :: taug(:,:,:), fracs(:,:,:)                  ! (ncol,nlay,ngptlw)
      real(kind=rb), intent(out), optional, target :: planklay(:,:,:)                   ! (ncol,nlay,nbndlw)
      real(kind=rb), intent(out), optional, target :: planklev(:,:,:)                   ! (ncol,0:nlay,nbndlw)
      real(kind=rb), intent(out), optional, target :: plankbnd(:,:), dplankbnd_dt(:,:)  ! (ncol,nbndlw)

      integer(c_int) :: rc, idrv, ng
      real(c_double), allocatable, target :: t1(:,:,:), t2(:,:,:), t3(:,:,:), t4(:,:,:), t5(:,:), t6(:,:)
      type(c_ptr) :: p1, p2, p3, p4, p5, p6

      ng = rrtmg_lw_hip_gpoints()
      call check_extent('play', size(play,1), size(play,2), ncol, nlay)
      call check_extent('plev', size(plev,1), size(plev,2), ncol, nlay+1)
      call check_extent('emis', size(emis,1), size(emis,2), ncol, 16)
      call out3('taug', taug, t1, p1, ncol, nlay, ng)
      call out3('fracs', fracs, t2, p2, ncol, nlay, ng)
      p3 = c_null_ptr; p4 = c_null_ptr; p5 = c_null_ptr; p6 = c_null_ptr
      if (present(planklay)) call out3('planklay', planklay, t3, p3, ncol, nlay, 16)
      if (present(planklev)) call out3('planklev', planklev, t4, p4, ncol, nlay+1, 16)
      if (present(plankbnd)) call out2('plankbnd', plankbnd, t5, p5, ncol)
      if (present(dplankbnd_dt)) call out2('dplankbnd_dt', dplankbnd_dt, t6, p6, ncol)
      idrv = merge(1, 0, present(dplankbnd_dt))
      rc = rrtmg_lw_hip_gas_optics(int(ncol, c_int), int(nlay, c_int), idrv, &
            play(1:ncol,1:nlay), plev(1:ncol,1:nlay+1), tlay(1:ncol,1:nlay), tlev(1:ncol,1:nlay+1), tsfc(1:ncol), &
            h2ovmr(1:ncol,1:nlay), o3vmr(1:ncol,1:nlay), co2vmr(1:ncol,1:nlay), ch4vmr(1:ncol,1:nlay), &
            n2ovmr(1:ncol,1:nlay), o2vmr(1:ncol,1:nlay), cfc11vmr(1:ncol,1:nlay), cfc12vmr(1:ncol,1:nlay), &
            cfc22vmr(1:ncol,1:nlay), ccl4vmr(1:ncol,1:nlay), emis(1:ncol,1:16), p1, p2, p3, p4, p5, p6)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_gas_optics')
      if (allocated(t1)) taug(1:ncol, 1:nlay, 1:ng) = t1
      if (allocated(t2)) fracs(1:ncol, 1:nlay, 1:ng) = t2
      if (allocated(t3)) planklay(1:ncol, 1:nlay, 1:16) = t3
      if (allocated(t4)) planklev(1:ncol, 1:nlay+1, 1:16) = t4
      if (allocated(t5)) plankbnd(1:ncol, 1:16) = t5
      if (allocated(t6)) dplankbnd_dt(1:ncol, 1:16) = t6

      end subroutine rrtmg_lw_gas_optics

      subroutine rrtmg_lw_cloud_optics &
            (ncol    ,nlay    ,imca    ,inflglw ,iceflglw,liqflglw, &
             cldfr   ,taucld  ,cicewp  ,cliqwp  ,reice   ,reliq   , &
             plev    ,h2ovmr  ,taucloud,ncbands ,secdiff)

      integer(kind=im), intent(in) :: ncol, nlay
      integer(kind=im), intent(in) :: imca            ! 0: cldprop, 1: cldprmc on a cloudy sub-column
      integer(kind=im), intent(in) :: inflglw, iceflglw, liqflglw
      real(kind=rb), intent(in) :: cldfr(:,:)         ! Cloud fraction                      (ncol,nlay)
      real(kind=rb), intent(in) :: taucld(:,:,:)      ! In-cloud optical depth              (nbndlw,ncol,nlay)
      real(kind=rb), intent(in) :: cicewp(:,:), cliqwp(:,:), reice(:,:), reliq(:,:)
      real(kind=rb), intent(in), optional :: plev(:,:), h2ovmr(:,:)                     ! (ncol,nlay+1), (ncol,nlay): with secdiff
      real(kind=rb), intent(out), optional, target :: taucloud(:,:,:)                   ! (ncol,nlay,nbndlw)
      integer(kind=im), intent(out), optional :: ncbands(:)                             ! (ncol)
      real(kind=rb), intent(out), optional, target :: secdiff(:,:)                      ! (ncol,nbndlw)

      integer(c_int) :: rc
      real(c_double), allocatable, target :: t1(:,:,:), t3(:,:), hp(:,:), hh(:,:)
      integer(c_int), allocatable, target :: nb(:)
      type(c_ptr) :: p1, p2, p3, pp, ph

      call check_extent('cldfr', size(cldfr,1), size(cldfr,2), ncol, nlay)
      call check_extent('taucld', size(taucld,2), size(taucld,3), ncol, nlay)
      p1 = c_null_ptr; p2 = c_null_ptr; p3 = c_null_ptr; pp = c_null_ptr; ph = c_null_ptr
      if (present(taucloud)) call out3('taucloud', taucloud, t1, p1, ncol, nlay, 16)
      if (present(ncbands)) then
         if (size(ncbands) < ncol) then
            write(*,'(a)') 'rrtmg_lw_cloud_optics: ncbands smaller than (ncol)'
            error stop 1
         endif
         allocate(nb(ncol))
         p2 = c_loc(nb)
      endif
      if (present(secdiff)) then
         if (.not. (present(plev) .and. present(h2ovmr))) then
            write(*,'(a)') 'rrtmg_lw_cloud_optics: secdiff needs plev and h2ovmr'
            error stop 1
         endif
         call check_extent('plev', size(plev,1), size(plev,2), ncol, nlay+1)
         call check_extent('h2ovmr', size(h2ovmr,1), size(h2ovmr,2), ncol, nlay)
         call out2('secdiff', secdiff, t3, p3, ncol)
         allocate(hp(ncol, nlay+1), hh(ncol, nlay))
         hp = plev(1:ncol, 1:nlay+1)
         hh = h2ovmr(1:ncol, 1:nlay)
         pp = c_loc(hp); ph = c_loc(hh)
      endif
      rc = rrtmg_lw_hip_cloud_optics(int(ncol, c_int), int(nlay, c_int), int(imca, c_int), int(inflglw, c_int), int(iceflglw, c_int), &
            int(liqflglw, c_int), cldfr(1:ncol,1:nlay), taucld(1:16,1:ncol,1:nlay), cicewp(1:ncol,1:nlay), cliqwp(1:ncol,1:nlay), &
            reice(1:ncol,1:nlay), reliq(1:ncol,1:nlay), pp, ph, p1, p2, p3)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_cloud_optics')
      if (allocated(t1)) taucloud(1:ncol, 1:nlay, 1:16) = t1
      if (allocated(nb)) ncbands(1:ncol) = int(nb, kind=im)
      if (allocated(t3)) secdiff(1:ncol, 1:16) = t3

      end subroutine rrtmg_lw_cloud_optics

      subroutine rrtmg_lw_solve &
            (ncol    ,nlay    ,cloud   , &
             plev    ,emis    ,tau     ,fracs   , &
             planklay,planklev,plankbnd, &
             uflx    ,dflx    ,hr      ,uflxc   ,dflxc   ,hrc     , &
             dplankbnd_dt,duflx_dt,duflxc_dt, &
             cldfr   ,odcld   ,submask)

      integer(kind=im), intent(in) :: ncol, nlay
      integer(kind=im), intent(in) :: cloud           ! 0: no cloud, 1: rtrn (cldfr, odcld), 2: rtrnmc (submask, odcld)
      real(kind=rb), intent(in) :: plev(:,:)          ! Interface pressures (hPa, mb)       (ncol,nlay+1)
      real(kind=rb), intent(in) :: emis(:,:)          ! Surface emissivity                  (ncol,nbndlw)
      real(kind=rb), intent(in) :: tau(:,:,:)         ! Clear-sky optical depth along the diffusivity path (ncol,nlay,ngptlw)
      real(kind=rb), intent(in) :: fracs(:,:,:)       ! Planck fractions                    (ncol,nlay,ngptlw)
      real(kind=rb), intent(in) :: planklay(:,:,:)    ! (ncol,nlay,nbndlw)
      real(kind=rb), intent(in) :: planklev(:,:,:)    ! (ncol,0:nlay,nbndlw)
      real(kind=rb), intent(in) :: plankbnd(:,:)      ! (ncol,nbndlw)
      real(kind=rb), intent(out), target :: uflx(:,:), dflx(:,:)                        ! (ncol,nlay+1)
      real(kind=rb), intent(out), target :: hr(:,:)                                     ! (ncol,nlay)
      real(kind=rb), intent(out), optional, target :: uflxc(:,:), dflxc(:,:), hrc(:,:)  ! all three or none
      real(kind=rb), intent(in), optional :: dplankbnd_dt(:,:)                          ! (ncol,nbndlw): with duflx_dt
      real(kind=rb), intent(out), optional, target :: duflx_dt(:,:), duflxc_dt(:,:)     ! (ncol,nlay+1): present = idrv 1
      real(kind=rb), intent(in), optional :: cldfr(:,:)                                 ! (ncol,nlay): cloud = 1
      real(kind=rb), intent(in), optional :: odcld(:,:,:)                               ! (ncol,nlay,nbndlw): cloud = 1, 2
      integer(c_int), intent(in), optional :: submask(:,:,:)                            ! (ncol,nlay,(ngptlw+31)/32): cloud = 2

      integer(c_int) :: rc, idrv, ng, mw
      real(c_double), allocatable, target :: t(:,:,:)            ! the outputs' temporaries, one plane each
      real(c_double), allocatable, target :: hd(:,:), hc(:,:), ho(:,:,:)
      integer(c_int), allocatable, target :: hm(:,:,:)
      type(c_ptr) :: p(8), pd, pc, po, pm
      logical :: tmp(8)

      ng = rrtmg_lw_hip_gpoints()
      mw = (ng + 31) / 32
      call check_extent('plev', size(plev,1), size(plev,2), ncol, nlay+1)
      call check_extent('emis', size(emis,1), size(emis,2), ncol, 16)
      call check_extent('plankbnd', size(plankbnd,1), size(plankbnd,2), ncol, 16)
      call check_extent('tau', size(tau,1), size(tau,2), ncol, nlay)
      call check_extent('fracs', size(fracs,1), size(fracs,2), ncol, nlay)
      call check_extent('planklay', size(planklay,1), size(planklay,2), ncol, nlay)
      call check_extent('planklev', size(planklev,1), size(planklev,2), ncol, nlay+1)
      idrv = merge(1, 0, present(duflx_dt))
      p = c_null_ptr; pd = c_null_ptr; pc = c_null_ptr; po = c_null_ptr; pm = c_null_ptr
      tmp = .false.
      allocate(t(ncol, nlay+1, 8))
      call outl('uflx', uflx, 1, nlay+1)
      call outl('dflx', dflx, 2, nlay+1)
      call outl('hr', hr, 3, nlay)
      if (present(uflxc)) call outl('uflxc', uflxc, 4, nlay+1)
      if (present(dflxc)) call outl('dflxc', dflxc, 5, nlay+1)
      if (present(hrc)) call outl('hrc', hrc, 6, nlay)
      if (present(duflx_dt)) call outl('duflx_dt', duflx_dt, 7, nlay+1)
      if (present(duflxc_dt)) call outl('duflxc_dt', duflxc_dt, 8, nlay+1)
      if (present(dplankbnd_dt)) then
         call check_extent('dplankbnd_dt', size(dplankbnd_dt,1), size(dplankbnd_dt,2), ncol, 16)
         allocate(hd(ncol, 16))
         hd = dplankbnd_dt(1:ncol, 1:16)
         pd = c_loc(hd)
      endif
      if (present(cldfr)) then
         call check_extent('cldfr', size(cldfr,1), size(cldfr,2), ncol, nlay)
         allocate(hc(ncol, nlay))
         hc = cldfr(1:ncol, 1:nlay)
         pc = c_loc(hc)
      endif
      if (present(odcld)) then
         call check_extent('odcld', size(odcld,1), size(odcld,2), ncol, nlay)
         allocate(ho(ncol, nlay, 16))
         ho = odcld(1:ncol, 1:nlay, 1:16)
         po = c_loc(ho)
      endif
      if (present(submask)) then
         call check_extent('submask', size(submask,1), size(submask,2), ncol, nlay)
         allocate(hm(ncol, nlay, mw))
         hm = submask(1:ncol, 1:nlay, 1:mw)
         pm = c_loc(hm)
      endif
      rc = rrtmg_lw_hip_solve(int(ncol, c_int), int(nlay, c_int), int(cloud, c_int), idrv, &
            plev(1:ncol,1:nlay+1), emis(1:ncol,1:16), tau(1:ncol,1:nlay,1:ng), fracs(1:ncol,1:nlay,1:ng), &
            planklay(1:ncol,1:nlay,1:16), planklev(1:ncol,1:nlay+1,1:16), plankbnd(1:ncol,1:16), pd, pc, po, pm, &
            p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8))
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_solve')
      if (tmp(1)) uflx(1:ncol, 1:nlay+1) = t(:, :, 1)
      if (tmp(2)) dflx(1:ncol, 1:nlay+1) = t(:, :, 2)
      if (tmp(3)) hr(1:ncol, 1:nlay) = t(:, 1:nlay, 3)
      if (tmp(4)) uflxc(1:ncol, 1:nlay+1) = t(:, :, 4)
      if (tmp(5)) dflxc(1:ncol, 1:nlay+1) = t(:, :, 5)
      if (tmp(6)) hrc(1:ncol, 1:nlay) = t(:, 1:nlay, 6)
      if (tmp(7)) duflx_dt(1:ncol, 1:nlay+1) = t(:, :, 7)
      if (tmp(8)) duflxc_dt(1:ncol, 1:nlay+1) = t(:, :, 8)

      contains

      ! output k, (ncol,n2): an exactly sized, contiguous actual goes across in place, a larger or strided one through plane k of t
      ! (its first ncol x n2 elements: the C entry's layout), copied back after the call
      subroutine outl(name, a, k, n2)
      character(len=*), intent(in) :: name
      real(kind=rb), intent(inout), target :: a(:,:)
      integer, intent(in) :: k
      integer(kind=im), intent(in) :: n2
      call check_extent(name, size(a,1), size(a,2), ncol, n2)
      if (size(a,1) == ncol .and. size(a,2) == n2 .and. is_contiguous(a)) then
         p(k) = c_loc(a)
      else
         tmp(k) = .true.
         p(k) = c_loc(t(1, 1, k))
      endif
      end subroutine outl

      end subroutine rrtmg_lw_solve

      ! an output (n1,n2,n3): exactly sized, contiguous actuals go across in place; larger or strided ones through the temporary t,
      ! copied back after the call
      subroutine out3(name, a, t, p, n1, n2, n3)
      character(len=*), intent(in) :: name
      real(kind=rb), intent(inout), target :: a(:,:,:)
      real(c_double), allocatable, target, intent(inout) :: t(:,:,:)
      type(c_ptr), intent(out) :: p
      integer, intent(in) :: n1, n2, n3
      if (size(a,1) < n1 .or. size(a,2) < n2 .or. size(a,3) < n3) then
         write(*,'(a,a,a,i0,a,i0,a,i0,a)') 'rrtmg_lw_gas_optics: ', name, ' smaller than (', n1, ',', n2, ',', n3, ')'
         error stop 1
      endif
      if (size(a,1) == n1 .and. size(a,2) == n2 .and. size(a,3) == n3 .and. is_contiguous(a)) then
         p = c_loc(a)
      else
         allocate(t(n1, n2, n3))
         p = c_loc(t)
      endif
      end subroutine out3

      ! the same for an output (ncol,16)
      subroutine out2(name, a, t, p, ncol)
      character(len=*), intent(in) :: name
      real(kind=rb), intent(inout), target :: a(:,:)
      real(c_double), allocatable, target, intent(inout) :: t(:,:)
      type(c_ptr), intent(out) :: p
      integer(kind=im), intent(in) :: ncol
      call check_extent(name, size(a,1), size(a,2), ncol, 16)
      if (size(a,1) == ncol .and. size(a,2) == 16 .and. is_contiguous(a)) then
         p = c_loc(a)
      else
         allocate(t(ncol, 16))
         p = c_loc(t)
      endif
      end subroutine out2

      subroutine check_extent(name, n1, n2, ncol, nl)
      character(len=*), intent(in) :: name
      integer, intent(in) :: n1, n2
      integer(kind=im), intent(in) :: ncol, nl
      if (n1 < ncol .or. n2 < nl) then
         write(*,'(a,a,a,i0,a,i0,a,i0,a,i0,a)') 'rrtmg_lw_gas_optics: ', name, ' has extents (', n1, ',', n2, &
               '), smaller than (', ncol, ',', nl, ')'
         error stop 1
      endif
      end subroutine check_extent

      end module rrtmg_lw_optics
