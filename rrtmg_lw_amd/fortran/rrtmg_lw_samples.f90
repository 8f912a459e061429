!  The mean over several sub-column samples (this library's extension; include/rrtmg_lw_hip.h, "The mean over several sub-column
!  samples"):
!      use rrtmg_lw_samples, only: rrtmg_lw_mcica_samples
!      call rrtmg_lw_mcica_samples(ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, &
!                                  play, plev, tlay, tlev, tsfc, h2ovmr, ..., ccl4vmr, emis, inflglw, iceflglw, liqflglw, &
!                                  cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, &
!                                  uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt [, uflx_var, dflx_var, hr_var])
!  mcica_subcol_lw + the McICA rrtmg_lw, nsamp times with the seeds permuteseed + s * seedstep (s = 0 .. nsamp-1; seedstep = the
!  sub-columns of a sample, 140, is the choice src/mcica_subcol_gen_lw.f90:193-196 documents), in one call: uflx, dflx, hr and duflx_dt
!  come back as the mean over the samples (float64 sum in sample order, one division), the clear-sky outputs as those of sample 0.
!  The arguments are the fused C entry's in its order: real(8) host arrays of exactly the declared shapes, the generator's cloud inputs
!  (cldfr, cicewp, cliqwp, reice, reliq, alpha (ncol,nlay), taucld (16,ncol,nlay)), tauaer (ncol,nlay,16).  icld and irng are in/out as
!  there; irng must be 0 (kissvec) with nsamp > 1.  The optional uflx_var, dflx_var (ncol,nlay+1) and hr_var (ncol,nlay) receive the
!  unbiased sample variances of uflx, dflx and hr (nsamp > 1; rrtmg_lw_hip_run_mcica_samples_var): sqrt(var / nsamp) is the standard
!  error of the mean.  duflx_dt and duflxc_dt are written with idrv = 1 only.  A refusal stops the program
!  with the library's text, like the other modules' entries.
      module rrtmg_lw_samples

      use iso_c_binding
      use parkind, only : im => kind_im, rb => kind_rb
      use rrtmg_lw_init, only : rrtmg_lw_hip_abort

      implicit none

      public :: rrtmg_lw_mcica_samples

      interface
         function rrtmg_lw_hip_run_mcica_samples(ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, &
               play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, &
               emis, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt) bind(C, name='rrtmg_lw_hip_run_mcica_samples') result(rc)
            import :: c_int, c_double
            integer(c_int), value :: ncol, nlay, idrv, permuteseed, nsamp, seedstep, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld, irng
            real(c_double), intent(in) :: play(*), plev(*), tlay(*), tlev(*), tsfc(*), h2ovmr(*), o3vmr(*), co2vmr(*), ch4vmr(*), &
                  n2ovmr(*), o2vmr(*), cfc11vmr(*), cfc12vmr(*), cfc22vmr(*), ccl4vmr(*), emis(*), cldfr(*), taucld(*), cicewp(*), &
                  cliqwp(*), reice(*), reliq(*), alpha(*), tauaer(*)
            real(c_double), intent(inout) :: uflx(*), dflx(*), hr(*), uflxc(*), dflxc(*), hrc(*), duflx_dt(*), duflxc_dt(*)
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_mcica_samples
         function rrtmg_lw_hip_run_mcica_samples_var(ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, &
               play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, &
               emis, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var) &
               bind(C, name='rrtmg_lw_hip_run_mcica_samples_var') result(rc)
            import :: c_int, c_double, c_ptr
            integer(c_int), value :: ncol, nlay, idrv, permuteseed, nsamp, seedstep, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld, irng
            real(c_double), intent(in) :: play(*), plev(*), tlay(*), tlev(*), tsfc(*), h2ovmr(*), o3vmr(*), co2vmr(*), ch4vmr(*), &
                  n2ovmr(*), o2vmr(*), cfc11vmr(*), cfc12vmr(*), cfc22vmr(*), ccl4vmr(*), emis(*), cldfr(*), taucld(*), cicewp(*), &
                  cliqwp(*), reice(*), reliq(*), alpha(*), tauaer(*)
            real(c_double), intent(inout) :: uflx(*), dflx(*), hr(*), uflxc(*), dflxc(*), hrc(*), duflx_dt(*), duflxc_dt(*)
            type(c_ptr), value :: uflx_var, dflx_var, hr_var          ! (each may be null)
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_mcica_samples_var
      end interface

      contains

      subroutine rrtmg_lw_mcica_samples &
            (ncol    ,nlay    ,icld    ,idrv    ,permuteseed, nsamp, seedstep, irng, &
             play    ,plev    ,tlay    ,tlev    ,tsfc    , &
             h2ovmr  ,o3vmr   ,co2vmr  ,ch4vmr  ,n2ovmr  ,o2vmr , &
             cfc11vmr,cfc12vmr,cfc22vmr,ccl4vmr ,emis    , &
             inflglw ,iceflglw,liqflglw, &
             cldfr   ,taucld  ,cicewp  ,cliqwp  ,reice   ,reliq , alpha, tauaer, &
             uflx    ,dflx    ,hr      ,uflxc   ,dflxc   ,hrc   , duflx_dt, duflxc_dt, &
             uflx_var,dflx_var,hr_var)

      integer(kind=im), intent(in) :: ncol            ! Number of horizontal columns
      integer(kind=im), intent(in) :: nlay            ! Number of model layers
      integer(kind=im), intent(inout) :: icld         ! Cloud overlap method of the generator (0 .. 5); comes back as rrtmg_lw leaves it
      integer(kind=im), intent(in) :: idrv            ! 1: the derivatives of the upward fluxes as well
      integer(kind=im), intent(in) :: permuteseed     ! Seed of sample 0
      integer(kind=im), intent(in) :: nsamp           ! Number of samples (1 .. 64)
      integer(kind=im), intent(in) :: seedstep        ! Seed of sample s: permuteseed + s * seedstep
      integer(kind=im), intent(inout) :: irng         ! Random number generator: 0 kissvec (required with nsamp > 1)
      real(kind=rb), intent(in) :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol)
      real(kind=rb), intent(in) :: h2ovmr(ncol,nlay), o3vmr(ncol,nlay), co2vmr(ncol,nlay), ch4vmr(ncol,nlay), n2ovmr(ncol,nlay)
      real(kind=rb), intent(in) :: o2vmr(ncol,nlay), cfc11vmr(ncol,nlay), cfc12vmr(ncol,nlay), cfc22vmr(ncol,nlay), ccl4vmr(ncol,nlay)
      real(kind=rb), intent(in) :: emis(ncol,16)
      integer(kind=im), intent(in) :: inflglw, iceflglw, liqflglw
      real(kind=rb), intent(in) :: cldfr(ncol,nlay), taucld(16,ncol,nlay), cicewp(ncol,nlay), cliqwp(ncol,nlay)
      real(kind=rb), intent(in) :: reice(ncol,nlay), reliq(ncol,nlay), alpha(ncol,nlay), tauaer(ncol,nlay,16)
      real(kind=rb), intent(inout) :: uflx(ncol,nlay+1), dflx(ncol,nlay+1), hr(ncol,nlay)          ! means over the samples
      real(kind=rb), intent(inout) :: uflxc(ncol,nlay+1), dflxc(ncol,nlay+1), hrc(ncol,nlay)       ! clear sky: sample 0
      real(kind=rb), intent(inout) :: duflx_dt(ncol,nlay+1), duflxc_dt(ncol,nlay+1)                ! written with idrv = 1
      ! unbiased sample variances of uflx, dflx, hr over the samples (nsamp > 1), each on its own
      real(kind=rb), intent(inout), optional, target :: uflx_var(ncol,nlay+1), dflx_var(ncol,nlay+1), hr_var(ncol,nlay)

      integer(c_int) :: rc, icld_c, irng_c
      type(c_ptr) :: pv(3)

      icld_c = int(icld, c_int)
      irng_c = int(irng, c_int)
      pv = c_null_ptr
      if (present(uflx_var)) pv(1) = c_loc(uflx_var)
      if (present(dflx_var)) pv(2) = c_loc(dflx_var)
      if (present(hr_var)) pv(3) = c_loc(hr_var)
      if (c_associated(pv(1)) .or. c_associated(pv(2)) .or. c_associated(pv(3))) then
      rc = rrtmg_lw_hip_run_mcica_samples_var(int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), int(permuteseed, c_int), &
            int(nsamp, c_int), int(seedstep, c_int), irng_c, play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, &
            o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), &
            cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, &
            pv(1), pv(2), pv(3))
      else
      rc = rrtmg_lw_hip_run_mcica_samples(int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), int(permuteseed, c_int), &
            int(nsamp, c_int), int(seedstep, c_int), irng_c, play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, &
            o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), &
            cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt)
      endif
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_mcica_samples')
      icld = int(icld_c, im)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_samples

      end module rrtmg_lw_samples
