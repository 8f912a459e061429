!  Cloud cover as the McICA sub-columns realise it (this library's extension; include/rrtmg_lw_hip.h, "Cloud cover as the McICA
!  sub-columns realise it"):
!      use rrtmg_lw_cover, only: rrtmg_lw_cloud_cover
!      call rrtmg_lw_cloud_cover(ncol, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr &
!                                [, alpha, cldtot, cldcum, cldlay, submask])
!  The generator stage of the fused McICA entries (module rrtmg_lw_rad's mcica_subcol_lw + rrtmg_lw, module rrtmg_lw_samples) with the
!  same icld, permuteseed, irng, play, cldfr and alpha, counted instead of solved: what comes back is exactly the cloud those calls saw.
!  With NG = 140 sub-columns and nsamp samples drawn with the seeds permuteseed + s * seedstep (s = 0 .. nsamp-1):
!      cldtot (ncol)           share of the NG * nsamp sub-columns with cloud in at least one layer
!      cldcum (ncol,nlay)      ... with cloud in layer k or any layer above it (layer 1 at the surface): cldcum(:,1) = cldtot; high /
!                              mid / low cover as seen from above are differences of its columns
!      cldlay (ncol,nlay)      ... with cloud in layer k: the realised layer fraction
!      submask (ncol,nlay,mw)  integer(4), mw = (NG + 31) / 32 = 5: bit mod(g, 32) of word g / 32 + 1 is set where sub-column g (0-based)
!                              of sample 0 is cloudy; nsamp = 1 only
!  The four are optional, each on its own; at least one must be present.  alpha (ncol,nlay) is needed with icld = 4 and 5 only.  Every
!  value is count / (NG * nsamp), ONE float64 division.  icld = 0 returns zeros.  irng is in/out (0 kissvec; any other value comes back
!  as 1, the Mersenne Twister, nsamp = 1 only).  Host arrays of exactly the declared shapes.  rrtmg_lw_cloud_cover is generic over the
!  real kind: real(4) arrays (a host built with 4-byte reals) are widened, the call is made in float64 and the results are rounded.
!  A refusal stops the program with the library's text, like the other modules' entries.  The device-resident form is
!  rrtmg_lw_cloud_cover_dev of module rrtmg_lw_device.
      module rrtmg_lw_cover

      use iso_c_binding
      use parkind, only : im => kind_im, rb => kind_rb
      use rrtmg_lw_init, only : rrtmg_lw_hip_abort

      implicit none

      private
      public :: rrtmg_lw_cloud_cover

      integer, parameter :: r4 = c_float

      interface rrtmg_lw_cloud_cover
         module procedure rrtmg_lw_cloud_cover_r8, rrtmg_lw_cloud_cover_r4
      end interface

      interface
         function rrtmg_lw_hip_mcica_cloud_cover(ncol, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, &
               cldtot, cldcum, cldlay, submask) bind(C, name='rrtmg_lw_hip_mcica_cloud_cover') result(rc)
            import :: c_int, c_ptr
            integer(c_int), value :: ncol, nlay, icld, permuteseed, nsamp, seedstep
            integer(c_int), intent(inout) :: irng
            type(c_ptr), value :: play, cldfr, alpha, cldtot, cldcum, cldlay, submask          ! (alpha and each output may be null)
            integer(c_int) :: rc
         end function rrtmg_lw_hip_mcica_cloud_cover
      end interface

      contains

      subroutine rrtmg_lw_cloud_cover_r8 &
            (ncol, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, cldtot, cldcum, cldlay, submask)

      integer(kind=im), intent(in) :: ncol            ! Number of horizontal columns
      integer(kind=im), intent(in) :: nlay            ! Number of model layers
      integer(kind=im), intent(in) :: icld            ! Cloud overlap method of the generator (0 .. 5)
      integer(kind=im), intent(in) :: permuteseed     ! Seed of sample 0
      integer(kind=im), intent(in) :: nsamp           ! Number of samples (1 .. 64)
      integer(kind=im), intent(in) :: seedstep        ! Seed of sample s: permuteseed + s * seedstep
      integer(kind=im), intent(inout) :: irng         ! Random number generator: 0 kissvec (required with nsamp > 1), 1 Mersenne Twister
      real(kind=rb), intent(in), target :: play(ncol,nlay)              ! Layer pressures (hPa, mb)
      real(kind=rb), intent(in), target :: cldfr(ncol,nlay)             ! Cloud fraction
      real(kind=rb), intent(in), optional, target :: alpha(ncol,nlay)   ! Overlap parameter (icld = 4, 5)
      real(kind=rb), intent(inout), optional, target :: cldtot(ncol), cldcum(ncol,nlay), cldlay(ncol,nlay)
      integer(c_int32_t), intent(inout), optional, target :: submask(ncol,nlay,*)

      integer(c_int) :: rc, irng_c
      type(c_ptr) :: p(5)

      p = c_null_ptr
      if (present(alpha)) p(1) = c_loc(alpha)
      if (present(cldtot)) p(2) = c_loc(cldtot)
      if (present(cldcum)) p(3) = c_loc(cldcum)
      if (present(cldlay)) p(4) = c_loc(cldlay)
      if (present(submask)) p(5) = c_loc(submask)
      irng_c = int(irng, c_int)
      rc = rrtmg_lw_hip_mcica_cloud_cover(int(ncol, c_int), int(nlay, c_int), int(icld, c_int), int(permuteseed, c_int), &
            int(nsamp, c_int), int(seedstep, c_int), irng_c, c_loc(play), c_loc(cldfr), p(1), p(2), p(3), p(4), p(5))
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_cloud_cover')
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_cloud_cover_r8

      ! the real(4) specific: the inputs widened (exact), the float64 call, the quotients rounded once
      subroutine rrtmg_lw_cloud_cover_r4 &
            (ncol, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, cldtot, cldcum, cldlay, submask)

      integer(kind=im), intent(in) :: ncol, nlay, icld, permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=r4), intent(in) :: play(ncol,nlay), cldfr(ncol,nlay)
      real(kind=r4), intent(in), optional :: alpha(ncol,nlay)
      real(kind=r4), intent(inout), optional :: cldtot(ncol), cldcum(ncol,nlay), cldlay(ncol,nlay)
      integer(c_int32_t), intent(inout), optional, target :: submask(ncol,nlay,*)

      integer(c_int) :: rc, irng_c
      type(c_ptr) :: p(5)
      real(c_double), allocatable, target :: wplay(:,:), wcldfr(:,:), walpha(:,:), wtot(:), wcum(:,:), wlay(:,:)

      allocate(wplay(ncol,nlay), wcldfr(ncol,nlay))
      wplay = real(play, c_double)
      wcldfr = real(cldfr, c_double)
      p = c_null_ptr
      if (present(alpha)) then
         allocate(walpha(ncol,nlay))
         walpha = real(alpha, c_double)
         p(1) = c_loc(walpha)
      endif
      if (present(cldtot)) then
         allocate(wtot(ncol))
         p(2) = c_loc(wtot)
      endif
      if (present(cldcum)) then
         allocate(wcum(ncol,nlay))
         p(3) = c_loc(wcum)
      endif
      if (present(cldlay)) then
         allocate(wlay(ncol,nlay))
         p(4) = c_loc(wlay)
      endif
      if (present(submask)) p(5) = c_loc(submask)
      irng_c = int(irng, c_int)
      rc = rrtmg_lw_hip_mcica_cloud_cover(int(ncol, c_int), int(nlay, c_int), int(icld, c_int), int(permuteseed, c_int), &
            int(nsamp, c_int), int(seedstep, c_int), irng_c, c_loc(wplay), c_loc(wcldfr), p(1), p(2), p(3), p(4), p(5))
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_cloud_cover')
      irng = int(irng_c, im)
      if (present(cldtot)) cldtot = real(wtot, r4)
      if (present(cldcum)) cldcum = real(wcum, r4)
      if (present(cldlay)) cldlay = real(wlay, r4)

      end subroutine rrtmg_lw_cloud_cover_r4

      end module rrtmg_lw_cover
