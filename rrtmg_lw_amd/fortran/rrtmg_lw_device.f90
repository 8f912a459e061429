!  Device-pointer entries for a GPU-resident Fortran host (this library's extension; include/rrtmg_lw_hip.h, "Device arrays with a column
!  stride"; INTEGRATION.md 4g):
!      use rrtmg_lw_device, only: rrtmg_lw_dev, rrtmg_lw_mcica_dev, rrtmg_lw_dtsfc_dev, rrtmg_lw_dev_check, rrtmg_lw_dev_status, &
!                                 rrtmg_lw_mcica_samples_dev, rrtmg_lw_alpha_dev, rrtmg_lw_cloud_cover_dev, rrtmg_lw_cloud_optics_dev
!      call rrtmg_lw_dev(ncol, ld, nlay, icld, idrv, play, plev, ..., uflx, dflx, hr, uflxc, dflxc, hrc &
!                        [, duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream])
!      call rrtmg_lw_dev_check([stream])
!  rrtmg_lw's argument list (module rrtmg_lw_rad) with ld behind ncol: every array lives in DEVICE memory - the host's own fields inside
!  an OpenACC host_data use_device region, an OpenMP target data use_device_addr region, or memory from hipMalloc behind c_f_pointer - and
!  is dimensioned (ld, .) with ld >= ncol, a host model's (pcols, pver) fields with ncol <= pcols:
!      play(ld,*) ... hr(ld,*)      emis(ld,*)      taucld(16,ld,*)      tauaer(ld,nlay,*)      uflxs(ld,nlay+1,*)      tsfc(*)
!  The routines take the ADDRESS of each dummy (c_loc) and hand it to rrtmg_lw_hip_run_nomcica_device_view; no dummy is ever read,
!  written, sized or copied on the host.  The call is enqueued on `stream` (a hipStream_t as type(c_ptr); absent: the default stream) and
!  returns at once: rrtmg_lw_dev_check(stream) waits for the stream and ends like the host shims on a physics error (rrtmg_lw_hip_abort:
!  the library's text, error stop); rrtmg_lw_dev_status(stream) returns the code instead (0: fine; the text: rrtmg_lw_hip_last_error).
!  An argument error of the enqueueing call itself ends through rrtmg_lw_hip_abort as well.  icld comes back as rrtmg_lw leaves it.
!
!  Two ways to pass the arrays, both under the same generic names:
!    * the array NAMES (rank as declared above: play(:,:) ...), for columns 1 .. ncol of the fields;
!    * the ELEMENT of the first column of the call in every array - play(c0,1), tsfc(c0), emis(c0,1), taucld(1,c0,1), tauaer(c0,1,1),
!      uflxs(c0,1,1) - for columns c0 .. c0+ncol-1 of wider fields.  Fortran resolves a generic name by rank, so an element does not
!      match an array dummy: these calls go to specifics whose dummies are scalars, which take the same address.  All arrays of a call
!      are passed one way.  An actual must be simply contiguous (a whole array, a contiguous pointer, an element of one): for anything
!      else the compiler would pass a host copy.
!  The routines are generic over the real kind like the host shims: real(kind_rb) (8 bytes) and real(4) - real_bytes = 4 of the view:
!  every array of the call float32, inputs widened, the solver in float64, outputs rounded.
!      rrtmg_lw_mcica_dev(ncol, ld, nlay, icld, idrv, permuteseed, irng, play, ..., reliq, alpha, tauaer, uflx, ... [, stream])
!  is the fused sub-column generator + McICA solver (rrtmg_lw_hip_run_mcica_subcol_device_view): the cloud arguments are the generator's
!  grid-mean inputs, alpha (ld,*) is optional (needed for icld = 4 and 5: pass it by keyword or in its place), irng comes back as 0 / 1.
!      rrtmg_lw_dtsfc_dev(ncol, ld, nlay, plev, dtsfc, uflx, dflx, duflx_dt, uflx_adj, hr_adj &
!                         [, uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj, stream])
!  is rrtmg_lw_dtsfc (module rrtmg_lw_adjust) on device arrays (rrtmg_lw_hip_adjust_tsfc_device_view).
!      rrtmg_lw_mcica_samples_dev(ncol, ld, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, ..., reliq, alpha, tauaer, &
!                                 uflx, dflx, hr, uflxc, dflxc, hrc [, duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, stream])
!  is rrtmg_lw_mcica_dev averaged over nsamp samples with the seeds permuteseed + s * seedstep (rrtmg_lw_hip_run_mcica_samples_device_view;
!  module rrtmg_lw_samples states the mean): uflx, dflx, hr, duflx_dt are means, the clear-sky outputs sample 0's, and the optional
!  uflx_var, dflx_var (ld,*) and hr_var (ld,*) receive the unbiased sample variances of uflx, dflx, hr (nsamp > 1; the standard error
!  of a mean is sqrt(var / nsamp)).  irng must be 0 with nsamp > 1.  No spectral outputs.
!      rrtmg_lw_alpha_dev(ncol, ld, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac, alpha [, stream])
!  is get_alpha on device arrays (rrtmg_lw_hip_get_alpha_device_view): dz, cldfrac, alpha (ld,*), lat(*); alpha is what the two McICA
!  routines above take for icld = 4 and 5.  For any other icld alpha is left alone.
!      rrtmg_lw_cloud_cover_dev(ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr &
!                               [, alpha, cldtot, cldcum, cldlay, submask, stream])
!  is rrtmg_lw_cloud_cover (module rrtmg_lw_cover) on device arrays (rrtmg_lw_hip_mcica_cloud_cover_device_view): the cloud that
!  rrtmg_lw_mcica_dev / rrtmg_lw_mcica_samples_dev with the same icld, seeds, irng, play, cldfr and alpha see, counted.  play, cldfr,
!  alpha, cldcum, cldlay (ld,*), cldtot(*), submask(ld,nlay,*) integer(4); the outputs are optional, each on its own (pass them by
!  keyword), at least one must be present; submask with nsamp = 1 only.
!      rrtmg_lw_cloud_optics_dev(ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq &
!                                [, plev, h2ovmr, taucloud, ncbands, secdiff, stream])
!  is rrtmg_lw_cloud_optics (module rrtmg_lw_optics) on device arrays (rrtmg_lw_hip_cloud_optics_device_view): cldfr, cicewp, cliqwp,
!  reice, reliq, plev, h2ovmr (ld,*), taucld(16,ld,*), taucloud(ld,nlay,*), secdiff(ld,*), ncbands(*) integer(4); the outputs are
!  optional, each on its own (pass them by keyword), at least one must be present; secdiff needs plev and h2ovmr.
      module rrtmg_lw_device

      use iso_c_binding
      use parkind, only : im => kind_im, rb => kind_rb
      use rrtmg_lw_init, only : rrtmg_lw_hip_abort

      implicit none

      private
      public :: rrtmg_lw_dev, rrtmg_lw_mcica_dev, rrtmg_lw_dtsfc_dev, rrtmg_lw_dev_check, rrtmg_lw_dev_status
      public :: rrtmg_lw_mcica_samples_dev, rrtmg_lw_alpha_dev, rrtmg_lw_cloud_cover_dev, rrtmg_lw_cloud_optics_dev

      integer, parameter :: r4 = c_float

      interface rrtmg_lw_dev
         module procedure rrtmg_lw_dev_r8, rrtmg_lw_dev_r4, rrtmg_lw_dev_r8_at, rrtmg_lw_dev_r4_at
      end interface
      interface rrtmg_lw_mcica_dev
         module procedure rrtmg_lw_mcica_dev_r8, rrtmg_lw_mcica_dev_r4, rrtmg_lw_mcica_dev_r8_at, rrtmg_lw_mcica_dev_r4_at
      end interface
      interface rrtmg_lw_dtsfc_dev
         module procedure rrtmg_lw_dtsfc_dev_r8, rrtmg_lw_dtsfc_dev_r4, rrtmg_lw_dtsfc_dev_r8_at, rrtmg_lw_dtsfc_dev_r4_at
      end interface

      interface rrtmg_lw_mcica_samples_dev
         module procedure rrtmg_lw_mcica_samples_dev_r8, rrtmg_lw_mcica_samples_dev_r4, rrtmg_lw_mcica_samples_dev_r8_at, rrtmg_lw_mcica_samples_dev_r4_at
      end interface
      interface rrtmg_lw_alpha_dev
         module procedure rrtmg_lw_alpha_dev_r8, rrtmg_lw_alpha_dev_r4, rrtmg_lw_alpha_dev_r8_at, rrtmg_lw_alpha_dev_r4_at
      end interface
      interface rrtmg_lw_cloud_cover_dev
         module procedure rrtmg_lw_cloud_cover_dev_r8, rrtmg_lw_cloud_cover_dev_r4, rrtmg_lw_cloud_cover_dev_r8_at, rrtmg_lw_cloud_cover_dev_r4_at
      end interface

      interface rrtmg_lw_cloud_optics_dev
         module procedure rrtmg_lw_cloud_optics_dev_r8, rrtmg_lw_cloud_optics_dev_r4, rrtmg_lw_cloud_optics_dev_r8_at, rrtmg_lw_cloud_optics_dev_r4_at
      end interface

      ! rrtmg_lw_hip_array_view
      type, bind(C) :: array_view
         integer(c_int) :: real_bytes, layer_fastest, top_first, ld
      end type array_view

      interface
         function rrtmg_lw_hip_run_nomcica_device_view(view, ncol, nlay, icld, idrv, play, plev, tlay, tlev, tsfc, &
               h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
               inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream) &
               bind(C, name='rrtmg_lw_hip_run_nomcica_device_view') result(rc)
            import :: c_int, c_ptr, array_view
            type(array_view), intent(in) :: view
            integer(c_int), value :: ncol, nlay, idrv, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld
            type(c_ptr), value :: play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr
            type(c_ptr), value :: cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer
            type(c_ptr), value :: uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_nomcica_device_view
         function rrtmg_lw_hip_run_mcica_subcol_device_view(view, ncol, nlay, icld, idrv, permuteseed, irng, play, plev, tlay, tlev, tsfc, &
               h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
               inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream) &
               bind(C, name='rrtmg_lw_hip_run_mcica_subcol_device_view') result(rc)
            import :: c_int, c_ptr, array_view
            type(array_view), intent(in) :: view
            integer(c_int), value :: ncol, nlay, idrv, permuteseed, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld, irng
            type(c_ptr), value :: play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr
            type(c_ptr), value :: cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer
            type(c_ptr), value :: uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_mcica_subcol_device_view
         function rrtmg_lw_hip_adjust_tsfc_device_view(view, ncol, nlay, plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt, &
               uflx_adj, hr_adj, uflxc_adj, hrc_adj, stream) bind(C, name='rrtmg_lw_hip_adjust_tsfc_device_view') result(rc)
            import :: c_int, c_ptr, array_view
            type(array_view), intent(in) :: view
            integer(c_int), value :: ncol, nlay
            type(c_ptr), value :: plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt, uflx_adj, hr_adj, uflxc_adj, hrc_adj, stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_adjust_tsfc_device_view
         function rrtmg_lw_hip_run_mcica_samples_device_view(view, ncol, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, &
               play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, &
               inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer, &
               uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, stream) &
               bind(C, name='rrtmg_lw_hip_run_mcica_samples_device_view') result(rc)
            import :: c_int, c_ptr, array_view
            type(array_view), intent(in) :: view
            integer(c_int), value :: ncol, nlay, idrv, permuteseed, nsamp, seedstep, inflglw, iceflglw, liqflglw
            integer(c_int), intent(inout) :: icld, irng
            type(c_ptr), value :: play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr
            type(c_ptr), value :: cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld, cicewp, cliqwp, reice, reliq, alpha, tauaer
            type(c_ptr), value :: uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_run_mcica_samples_device_view
         function rrtmg_lw_hip_get_alpha_device_view(view, ncol, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac, alpha, stream) &
               bind(C, name='rrtmg_lw_hip_get_alpha_device_view') result(rc)
            import :: c_int, c_double, c_ptr, array_view
            type(array_view), intent(in) :: view
            integer(c_int), value :: ncol, nlay, icld, idcor, juldat
            real(c_double), value :: decorr_con
            type(c_ptr), value :: dz, lat, cldfrac, alpha, stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_get_alpha_device_view
         function rrtmg_lw_hip_mcica_cloud_cover_device_view(view, ncol, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, &
               cldtot, cldcum, cldlay, submask, stream) bind(C, name='rrtmg_lw_hip_mcica_cloud_cover_device_view') result(rc)
            import :: c_int, c_ptr, array_view
            type(array_view), intent(in) :: view
            integer(c_int), value :: ncol, nlay, icld, permuteseed, nsamp, seedstep
            integer(c_int), intent(inout) :: irng
            type(c_ptr), value :: play, cldfr, alpha, cldtot, cldcum, cldlay, submask, stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_mcica_cloud_cover_device_view
         function rrtmg_lw_hip_cloud_optics_device_view(view, ncol, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, &
               reice, reliq, plev, h2ovmr, taucloud, ncbands, secdiff, stream) bind(C, name='rrtmg_lw_hip_cloud_optics_device_view') result(rc)
            import :: c_int, c_ptr, array_view
            type(array_view), intent(in) :: view
            integer(c_int), value :: ncol, nlay, imca, inflglw, iceflglw, liqflglw
            type(c_ptr), value :: cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr, taucloud, ncbands, secdiff, stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_cloud_optics_device_view
         function rrtmg_lw_hip_check(stream) bind(C, name='rrtmg_lw_hip_check') result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: stream
            integer(c_int) :: rc
         end function rrtmg_lw_hip_check
      end interface

      contains

      subroutine rrtmg_lw_dev_r8 &
            (ncol, ld, nlay, icld, idrv, play, plev, tlay, &
             tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, &
             cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, &
             cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, uflx, &
             dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, &
             dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      real(kind=rb), target :: play(ld,*), plev(ld,*), tlay(ld,*), tlev(ld,*), tsfc(*), h2ovmr(ld,*)
      real(kind=rb), target :: o3vmr(ld,*), co2vmr(ld,*), ch4vmr(ld,*), n2ovmr(ld,*), o2vmr(ld,*), cfc11vmr(ld,*)
      real(kind=rb), target :: cfc12vmr(ld,*), cfc22vmr(ld,*), ccl4vmr(ld,*), emis(ld,*), cldfr(ld,*), taucld(16,ld,*)
      real(kind=rb), target :: cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*), tauaer(ld,nlay,*)
      real(kind=rb), target :: uflx(ld,*), dflx(ld,*), hr(ld,*), uflxc(ld,*), dflxc(ld,*), hrc(ld,*)
      real(kind=rb), target, optional :: duflx_dt(ld,*), duflxc_dt(ld,*), uflxs(ld,nlay+1,*), dflxs(ld,nlay+1,*), uflxcs(ld,nlay+1,*), dflxcs(ld,nlay+1,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = 0
      call dev_solve('rrtmg_lw_dev', 8, .false., ncol, ld, nlay, icld, idrv, 0_c_int, irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)

      end subroutine rrtmg_lw_dev_r8

      subroutine rrtmg_lw_dev_r4 &
            (ncol, ld, nlay, icld, idrv, play, plev, tlay, &
             tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, &
             cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, &
             cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, uflx, &
             dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, &
             dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      real(kind=r4), target :: play(ld,*), plev(ld,*), tlay(ld,*), tlev(ld,*), tsfc(*), h2ovmr(ld,*)
      real(kind=r4), target :: o3vmr(ld,*), co2vmr(ld,*), ch4vmr(ld,*), n2ovmr(ld,*), o2vmr(ld,*), cfc11vmr(ld,*)
      real(kind=r4), target :: cfc12vmr(ld,*), cfc22vmr(ld,*), ccl4vmr(ld,*), emis(ld,*), cldfr(ld,*), taucld(16,ld,*)
      real(kind=r4), target :: cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*), tauaer(ld,nlay,*)
      real(kind=r4), target :: uflx(ld,*), dflx(ld,*), hr(ld,*), uflxc(ld,*), dflxc(ld,*), hrc(ld,*)
      real(kind=r4), target, optional :: duflx_dt(ld,*), duflxc_dt(ld,*), uflxs(ld,nlay+1,*), dflxs(ld,nlay+1,*), uflxcs(ld,nlay+1,*), dflxcs(ld,nlay+1,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = 0
      call dev_solve('rrtmg_lw_dev', 4, .false., ncol, ld, nlay, icld, idrv, 0_c_int, irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)

      end subroutine rrtmg_lw_dev_r4

      subroutine rrtmg_lw_dev_r8_at &
            (ncol, ld, nlay, icld, idrv, play, plev, tlay, &
             tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, &
             cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, &
             cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, uflx, &
             dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, &
             dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      real(kind=rb), target :: play, plev, tlay, tlev, tsfc, h2ovmr
      real(kind=rb), target :: o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr
      real(kind=rb), target :: cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld
      real(kind=rb), target :: cicewp, cliqwp, reice, reliq, tauaer
      real(kind=rb), target :: uflx, dflx, hr, uflxc, dflxc, hrc
      real(kind=rb), target, optional :: duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = 0
      call dev_solve('rrtmg_lw_dev', 8, .false., ncol, ld, nlay, icld, idrv, 0_c_int, irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)

      end subroutine rrtmg_lw_dev_r8_at

      subroutine rrtmg_lw_dev_r4_at &
            (ncol, ld, nlay, icld, idrv, play, plev, tlay, &
             tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, &
             cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, iceflglw, liqflglw, &
             cldfr, taucld, cicewp, cliqwp, reice, reliq, tauaer, uflx, &
             dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt, uflxs, &
             dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      real(kind=r4), target :: play, plev, tlay, tlev, tsfc, h2ovmr
      real(kind=r4), target :: o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr
      real(kind=r4), target :: cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld
      real(kind=r4), target :: cicewp, cliqwp, reice, reliq, tauaer
      real(kind=r4), target :: uflx, dflx, hr, uflxc, dflxc, hrc
      real(kind=r4), target, optional :: duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = 0
      call dev_solve('rrtmg_lw_dev', 4, .false., ncol, ld, nlay, icld, idrv, 0_c_int, irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)

      end subroutine rrtmg_lw_dev_r4_at

      subroutine rrtmg_lw_mcica_dev_r8 &
            (ncol, ld, nlay, icld, idrv, permuteseed, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed
      integer(kind=im), intent(inout) :: irng
      real(kind=rb), target :: play(ld,*), plev(ld,*), tlay(ld,*), tlev(ld,*), tsfc(*), h2ovmr(ld,*)
      real(kind=rb), target :: o3vmr(ld,*), co2vmr(ld,*), ch4vmr(ld,*), n2ovmr(ld,*), o2vmr(ld,*), cfc11vmr(ld,*)
      real(kind=rb), target :: cfc12vmr(ld,*), cfc22vmr(ld,*), ccl4vmr(ld,*), emis(ld,*), cldfr(ld,*), taucld(16,ld,*)
      real(kind=rb), target :: cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*), tauaer(ld,nlay,*)
      real(kind=rb), target, optional :: alpha(ld,*)
      real(kind=rb), target :: uflx(ld,*), dflx(ld,*), hr(ld,*), uflxc(ld,*), dflxc(ld,*), hrc(ld,*)
      real(kind=rb), target, optional :: duflx_dt(ld,*), duflxc_dt(ld,*), uflxs(ld,nlay+1,*), dflxs(ld,nlay+1,*), uflxcs(ld,nlay+1,*), dflxcs(ld,nlay+1,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = int(irng, c_int)
      call dev_solve('rrtmg_lw_mcica_dev', 8, .true., ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_dev_r8

      subroutine rrtmg_lw_mcica_dev_r4 &
            (ncol, ld, nlay, icld, idrv, permuteseed, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed
      integer(kind=im), intent(inout) :: irng
      real(kind=r4), target :: play(ld,*), plev(ld,*), tlay(ld,*), tlev(ld,*), tsfc(*), h2ovmr(ld,*)
      real(kind=r4), target :: o3vmr(ld,*), co2vmr(ld,*), ch4vmr(ld,*), n2ovmr(ld,*), o2vmr(ld,*), cfc11vmr(ld,*)
      real(kind=r4), target :: cfc12vmr(ld,*), cfc22vmr(ld,*), ccl4vmr(ld,*), emis(ld,*), cldfr(ld,*), taucld(16,ld,*)
      real(kind=r4), target :: cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*), tauaer(ld,nlay,*)
      real(kind=r4), target, optional :: alpha(ld,*)
      real(kind=r4), target :: uflx(ld,*), dflx(ld,*), hr(ld,*), uflxc(ld,*), dflxc(ld,*), hrc(ld,*)
      real(kind=r4), target, optional :: duflx_dt(ld,*), duflxc_dt(ld,*), uflxs(ld,nlay+1,*), dflxs(ld,nlay+1,*), uflxcs(ld,nlay+1,*), dflxcs(ld,nlay+1,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = int(irng, c_int)
      call dev_solve('rrtmg_lw_mcica_dev', 4, .true., ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_dev_r4

      subroutine rrtmg_lw_mcica_dev_r8_at &
            (ncol, ld, nlay, icld, idrv, permuteseed, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed
      integer(kind=im), intent(inout) :: irng
      real(kind=rb), target :: play, plev, tlay, tlev, tsfc, h2ovmr
      real(kind=rb), target :: o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr
      real(kind=rb), target :: cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld
      real(kind=rb), target :: cicewp, cliqwp, reice, reliq, tauaer
      real(kind=rb), target, optional :: alpha
      real(kind=rb), target :: uflx, dflx, hr, uflxc, dflxc, hrc
      real(kind=rb), target, optional :: duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = int(irng, c_int)
      call dev_solve('rrtmg_lw_mcica_dev', 8, .true., ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_dev_r8_at

      subroutine rrtmg_lw_mcica_dev_r4_at &
            (ncol, ld, nlay, icld, idrv, permuteseed, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed
      integer(kind=im), intent(inout) :: irng
      real(kind=r4), target :: play, plev, tlay, tlev, tsfc, h2ovmr
      real(kind=r4), target :: o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr
      real(kind=r4), target :: cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld
      real(kind=r4), target :: cicewp, cliqwp, reice, reliq, tauaer
      real(kind=r4), target, optional :: alpha
      real(kind=r4), target :: uflx, dflx, hr, uflxc, dflxc, hrc
      real(kind=r4), target, optional :: duflx_dt, duflxc_dt, uflxs, dflxs, uflxcs, dflxcs
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(12)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflxs)) pout(9) = c_loc(uflxs)
      if (present(dflxs)) pout(10) = c_loc(dflxs)
      if (present(uflxcs)) pout(11) = c_loc(uflxcs)
      if (present(dflxcs)) pout(12) = c_loc(dflxcs)
      irng_c = int(irng, c_int)
      call dev_solve('rrtmg_lw_mcica_dev', 4, .true., ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_dev_r4_at

      subroutine rrtmg_lw_dtsfc_dev_r8 &
            (ncol, ld, nlay, plev, dtsfc, uflx, dflx, duflx_dt, &
             uflx_adj, hr_adj, uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay
      real(kind=rb), target :: plev(ld,*), dtsfc(*), uflx(ld,*), dflx(ld,*), duflx_dt(ld,*), uflx_adj(ld,*)
      real(kind=rb), target :: hr_adj(ld,*)
      real(kind=rb), target, optional :: uflxc(ld,*), dflxc(ld,*), duflxc_dt(ld,*), uflxc_adj(ld,*), hrc_adj(ld,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(12)

      p = c_null_ptr
      p(1) = c_loc(plev)
      p(2) = c_loc(dtsfc)
      p(3) = c_loc(uflx)
      p(4) = c_loc(dflx)
      p(5) = c_loc(duflx_dt)
      if (present(uflxc)) p(6) = c_loc(uflxc)
      if (present(dflxc)) p(7) = c_loc(dflxc)
      if (present(duflxc_dt)) p(8) = c_loc(duflxc_dt)
      p(9) = c_loc(uflx_adj)
      p(10) = c_loc(hr_adj)
      if (present(uflxc_adj)) p(11) = c_loc(uflxc_adj)
      if (present(hrc_adj)) p(12) = c_loc(hrc_adj)
      call dev_adjust(8, ncol, ld, nlay, p, stream)

      end subroutine rrtmg_lw_dtsfc_dev_r8

      subroutine rrtmg_lw_dtsfc_dev_r4 &
            (ncol, ld, nlay, plev, dtsfc, uflx, dflx, duflx_dt, &
             uflx_adj, hr_adj, uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay
      real(kind=r4), target :: plev(ld,*), dtsfc(*), uflx(ld,*), dflx(ld,*), duflx_dt(ld,*), uflx_adj(ld,*)
      real(kind=r4), target :: hr_adj(ld,*)
      real(kind=r4), target, optional :: uflxc(ld,*), dflxc(ld,*), duflxc_dt(ld,*), uflxc_adj(ld,*), hrc_adj(ld,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(12)

      p = c_null_ptr
      p(1) = c_loc(plev)
      p(2) = c_loc(dtsfc)
      p(3) = c_loc(uflx)
      p(4) = c_loc(dflx)
      p(5) = c_loc(duflx_dt)
      if (present(uflxc)) p(6) = c_loc(uflxc)
      if (present(dflxc)) p(7) = c_loc(dflxc)
      if (present(duflxc_dt)) p(8) = c_loc(duflxc_dt)
      p(9) = c_loc(uflx_adj)
      p(10) = c_loc(hr_adj)
      if (present(uflxc_adj)) p(11) = c_loc(uflxc_adj)
      if (present(hrc_adj)) p(12) = c_loc(hrc_adj)
      call dev_adjust(4, ncol, ld, nlay, p, stream)

      end subroutine rrtmg_lw_dtsfc_dev_r4

      subroutine rrtmg_lw_dtsfc_dev_r8_at &
            (ncol, ld, nlay, plev, dtsfc, uflx, dflx, duflx_dt, &
             uflx_adj, hr_adj, uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay
      real(kind=rb), target :: plev, dtsfc, uflx, dflx, duflx_dt, uflx_adj
      real(kind=rb), target :: hr_adj
      real(kind=rb), target, optional :: uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(12)

      p = c_null_ptr
      p(1) = c_loc(plev)
      p(2) = c_loc(dtsfc)
      p(3) = c_loc(uflx)
      p(4) = c_loc(dflx)
      p(5) = c_loc(duflx_dt)
      if (present(uflxc)) p(6) = c_loc(uflxc)
      if (present(dflxc)) p(7) = c_loc(dflxc)
      if (present(duflxc_dt)) p(8) = c_loc(duflxc_dt)
      p(9) = c_loc(uflx_adj)
      p(10) = c_loc(hr_adj)
      if (present(uflxc_adj)) p(11) = c_loc(uflxc_adj)
      if (present(hrc_adj)) p(12) = c_loc(hrc_adj)
      call dev_adjust(8, ncol, ld, nlay, p, stream)

      end subroutine rrtmg_lw_dtsfc_dev_r8_at

      subroutine rrtmg_lw_dtsfc_dev_r4_at &
            (ncol, ld, nlay, plev, dtsfc, uflx, dflx, duflx_dt, &
             uflx_adj, hr_adj, uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay
      real(kind=r4), target :: plev, dtsfc, uflx, dflx, duflx_dt, uflx_adj
      real(kind=r4), target :: hr_adj
      real(kind=r4), target, optional :: uflxc, dflxc, duflxc_dt, uflxc_adj, hrc_adj
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(12)

      p = c_null_ptr
      p(1) = c_loc(plev)
      p(2) = c_loc(dtsfc)
      p(3) = c_loc(uflx)
      p(4) = c_loc(dflx)
      p(5) = c_loc(duflx_dt)
      if (present(uflxc)) p(6) = c_loc(uflxc)
      if (present(dflxc)) p(7) = c_loc(dflxc)
      if (present(duflxc_dt)) p(8) = c_loc(duflxc_dt)
      p(9) = c_loc(uflx_adj)
      p(10) = c_loc(hr_adj)
      if (present(uflxc_adj)) p(11) = c_loc(uflxc_adj)
      if (present(hrc_adj)) p(12) = c_loc(hrc_adj)
      call dev_adjust(4, ncol, ld, nlay, p, stream)

      end subroutine rrtmg_lw_dtsfc_dev_r4_at

      subroutine rrtmg_lw_mcica_samples_dev_r8 &
            (ncol, ld, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=rb), target :: play(ld,*), plev(ld,*), tlay(ld,*), tlev(ld,*), tsfc(*), h2ovmr(ld,*)
      real(kind=rb), target :: o3vmr(ld,*), co2vmr(ld,*), ch4vmr(ld,*), n2ovmr(ld,*), o2vmr(ld,*), cfc11vmr(ld,*)
      real(kind=rb), target :: cfc12vmr(ld,*), cfc22vmr(ld,*), ccl4vmr(ld,*), emis(ld,*), cldfr(ld,*), taucld(16,ld,*)
      real(kind=rb), target :: cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*), tauaer(ld,nlay,*)
      real(kind=rb), target, optional :: alpha(ld,*)
      real(kind=rb), target :: uflx(ld,*), dflx(ld,*), hr(ld,*), uflxc(ld,*), dflxc(ld,*), hrc(ld,*)
      real(kind=rb), target, optional :: duflx_dt(ld,*), duflxc_dt(ld,*), uflx_var(ld,*), dflx_var(ld,*), hr_var(ld,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(11)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflx_var)) pout(9) = c_loc(uflx_var)
      if (present(dflx_var)) pout(10) = c_loc(dflx_var)
      if (present(hr_var)) pout(11) = c_loc(hr_var)
      irng_c = int(irng, c_int)
      call dev_samples(8, ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), int(nsamp, c_int), int(seedstep, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_samples_dev_r8

      subroutine rrtmg_lw_mcica_samples_dev_r4 &
            (ncol, ld, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=r4), target :: play(ld,*), plev(ld,*), tlay(ld,*), tlev(ld,*), tsfc(*), h2ovmr(ld,*)
      real(kind=r4), target :: o3vmr(ld,*), co2vmr(ld,*), ch4vmr(ld,*), n2ovmr(ld,*), o2vmr(ld,*), cfc11vmr(ld,*)
      real(kind=r4), target :: cfc12vmr(ld,*), cfc22vmr(ld,*), ccl4vmr(ld,*), emis(ld,*), cldfr(ld,*), taucld(16,ld,*)
      real(kind=r4), target :: cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*), tauaer(ld,nlay,*)
      real(kind=r4), target, optional :: alpha(ld,*)
      real(kind=r4), target :: uflx(ld,*), dflx(ld,*), hr(ld,*), uflxc(ld,*), dflxc(ld,*), hrc(ld,*)
      real(kind=r4), target, optional :: duflx_dt(ld,*), duflxc_dt(ld,*), uflx_var(ld,*), dflx_var(ld,*), hr_var(ld,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(11)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflx_var)) pout(9) = c_loc(uflx_var)
      if (present(dflx_var)) pout(10) = c_loc(dflx_var)
      if (present(hr_var)) pout(11) = c_loc(hr_var)
      irng_c = int(irng, c_int)
      call dev_samples(4, ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), int(nsamp, c_int), int(seedstep, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_samples_dev_r4

      subroutine rrtmg_lw_mcica_samples_dev_r8_at &
            (ncol, ld, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=rb), target :: play, plev, tlay, tlev, tsfc, h2ovmr
      real(kind=rb), target :: o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr
      real(kind=rb), target :: cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld
      real(kind=rb), target :: cicewp, cliqwp, reice, reliq, tauaer
      real(kind=rb), target, optional :: alpha
      real(kind=rb), target :: uflx, dflx, hr, uflxc, dflxc, hrc
      real(kind=rb), target, optional :: duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(11)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflx_var)) pout(9) = c_loc(uflx_var)
      if (present(dflx_var)) pout(10) = c_loc(dflx_var)
      if (present(hr_var)) pout(11) = c_loc(hr_var)
      irng_c = int(irng, c_int)
      call dev_samples(8, ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), int(nsamp, c_int), int(seedstep, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_samples_dev_r8_at

      subroutine rrtmg_lw_mcica_samples_dev_r4_at &
            (ncol, ld, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, play, &
             plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, &
             n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis, inflglw, &
             iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, &
             alpha, tauaer, uflx, dflx, hr, uflxc, dflxc, hrc, &
             duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(kind=im), intent(in) :: permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=r4), target :: play, plev, tlay, tlev, tsfc, h2ovmr
      real(kind=r4), target :: o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr
      real(kind=r4), target :: cfc12vmr, cfc22vmr, ccl4vmr, emis, cldfr, taucld
      real(kind=r4), target :: cicewp, cliqwp, reice, reliq, tauaer
      real(kind=r4), target, optional :: alpha
      real(kind=r4), target :: uflx, dflx, hr, uflxc, dflxc, hrc
      real(kind=r4), target, optional :: duflx_dt, duflxc_dt, uflx_var, dflx_var, hr_var
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: pin(24), pout(11)
      integer(c_int) :: irng_c

      pin = c_null_ptr
      pout = c_null_ptr
      pin(1) = c_loc(play)
      pin(2) = c_loc(plev)
      pin(3) = c_loc(tlay)
      pin(4) = c_loc(tlev)
      pin(5) = c_loc(tsfc)
      pin(6) = c_loc(h2ovmr)
      pin(7) = c_loc(o3vmr)
      pin(8) = c_loc(co2vmr)
      pin(9) = c_loc(ch4vmr)
      pin(10) = c_loc(n2ovmr)
      pin(11) = c_loc(o2vmr)
      pin(12) = c_loc(cfc11vmr)
      pin(13) = c_loc(cfc12vmr)
      pin(14) = c_loc(cfc22vmr)
      pin(15) = c_loc(ccl4vmr)
      pin(16) = c_loc(emis)
      pin(17) = c_loc(cldfr)
      pin(18) = c_loc(taucld)
      pin(19) = c_loc(cicewp)
      pin(20) = c_loc(cliqwp)
      pin(21) = c_loc(reice)
      pin(22) = c_loc(reliq)
      pin(23) = c_loc(tauaer)
      if (present(alpha)) pin(24) = c_loc(alpha)
      pout(1) = c_loc(uflx)
      pout(2) = c_loc(dflx)
      pout(3) = c_loc(hr)
      pout(4) = c_loc(uflxc)
      pout(5) = c_loc(dflxc)
      pout(6) = c_loc(hrc)
      if (present(duflx_dt)) pout(7) = c_loc(duflx_dt)
      if (present(duflxc_dt)) pout(8) = c_loc(duflxc_dt)
      if (present(uflx_var)) pout(9) = c_loc(uflx_var)
      if (present(dflx_var)) pout(10) = c_loc(dflx_var)
      if (present(hr_var)) pout(11) = c_loc(hr_var)
      irng_c = int(irng, c_int)
      call dev_samples(4, ncol, ld, nlay, icld, idrv, int(permuteseed, c_int), int(nsamp, c_int), int(seedstep, c_int), irng_c, &
            inflglw, iceflglw, liqflglw, pin, pout, stream)
      irng = int(irng_c, im)

      end subroutine rrtmg_lw_mcica_samples_dev_r4_at

      subroutine rrtmg_lw_alpha_dev_r8 &
            (ncol, ld, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac, alpha, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, idcor, juldat
      real(kind=rb), intent(in) :: decorr_con
      real(kind=rb), target :: dz(ld,*), lat(*), cldfrac(ld,*), alpha(ld,*)
      type(c_ptr), intent(in), optional :: stream

      call dev_alpha(8, ncol, ld, nlay, icld, idcor, real(decorr_con, c_double), c_loc(dz), c_loc(lat), juldat, c_loc(cldfrac), &
            c_loc(alpha), stream)

      end subroutine rrtmg_lw_alpha_dev_r8

      subroutine rrtmg_lw_alpha_dev_r4 &
            (ncol, ld, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac, alpha, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, idcor, juldat
      real(kind=r4), intent(in) :: decorr_con
      real(kind=r4), target :: dz(ld,*), lat(*), cldfrac(ld,*), alpha(ld,*)
      type(c_ptr), intent(in), optional :: stream

      call dev_alpha(4, ncol, ld, nlay, icld, idcor, real(decorr_con, c_double), c_loc(dz), c_loc(lat), juldat, c_loc(cldfrac), &
            c_loc(alpha), stream)

      end subroutine rrtmg_lw_alpha_dev_r4

      subroutine rrtmg_lw_alpha_dev_r8_at &
            (ncol, ld, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac, alpha, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, idcor, juldat
      real(kind=rb), intent(in) :: decorr_con
      real(kind=rb), target :: dz, lat, cldfrac, alpha
      type(c_ptr), intent(in), optional :: stream

      call dev_alpha(8, ncol, ld, nlay, icld, idcor, real(decorr_con, c_double), c_loc(dz), c_loc(lat), juldat, c_loc(cldfrac), &
            c_loc(alpha), stream)

      end subroutine rrtmg_lw_alpha_dev_r8_at

      subroutine rrtmg_lw_alpha_dev_r4_at &
            (ncol, ld, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac, alpha, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, idcor, juldat
      real(kind=r4), intent(in) :: decorr_con
      real(kind=r4), target :: dz, lat, cldfrac, alpha
      type(c_ptr), intent(in), optional :: stream

      call dev_alpha(4, ncol, ld, nlay, icld, idcor, real(decorr_con, c_double), c_loc(dz), c_loc(lat), juldat, c_loc(cldfrac), &
            c_loc(alpha), stream)

      end subroutine rrtmg_lw_alpha_dev_r4_at

      subroutine rrtmg_lw_cloud_cover_dev_r8 &
            (ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, cldtot, cldcum, cldlay, submask, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=rb), target :: play(ld,*), cldfr(ld,*)
      real(kind=rb), target, optional :: alpha(ld,*), cldtot(*), cldcum(ld,*), cldlay(ld,*)
      integer(c_int32_t), target, optional :: submask(ld,nlay,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(5)

      p = c_null_ptr
      if (present(alpha)) p(1) = c_loc(alpha)
      if (present(cldtot)) p(2) = c_loc(cldtot)
      if (present(cldcum)) p(3) = c_loc(cldcum)
      if (present(cldlay)) p(4) = c_loc(cldlay)
      if (present(submask)) p(5) = c_loc(submask)
      call dev_cover(8, ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, c_loc(play), c_loc(cldfr), p, stream)

      end subroutine rrtmg_lw_cloud_cover_dev_r8

      subroutine rrtmg_lw_cloud_cover_dev_r4 &
            (ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, cldtot, cldcum, cldlay, submask, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=r4), target :: play(ld,*), cldfr(ld,*)
      real(kind=r4), target, optional :: alpha(ld,*), cldtot(*), cldcum(ld,*), cldlay(ld,*)
      integer(c_int32_t), target, optional :: submask(ld,nlay,*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(5)

      p = c_null_ptr
      if (present(alpha)) p(1) = c_loc(alpha)
      if (present(cldtot)) p(2) = c_loc(cldtot)
      if (present(cldcum)) p(3) = c_loc(cldcum)
      if (present(cldlay)) p(4) = c_loc(cldlay)
      if (present(submask)) p(5) = c_loc(submask)
      call dev_cover(4, ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, c_loc(play), c_loc(cldfr), p, stream)

      end subroutine rrtmg_lw_cloud_cover_dev_r4

      subroutine rrtmg_lw_cloud_cover_dev_r8_at &
            (ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, cldtot, cldcum, cldlay, submask, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=rb), target :: play, cldfr
      real(kind=rb), target, optional :: alpha, cldtot, cldcum, cldlay
      integer(c_int32_t), target, optional :: submask
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(5)

      p = c_null_ptr
      if (present(alpha)) p(1) = c_loc(alpha)
      if (present(cldtot)) p(2) = c_loc(cldtot)
      if (present(cldcum)) p(3) = c_loc(cldcum)
      if (present(cldlay)) p(4) = c_loc(cldlay)
      if (present(submask)) p(5) = c_loc(submask)
      call dev_cover(8, ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, c_loc(play), c_loc(cldfr), p, stream)

      end subroutine rrtmg_lw_cloud_cover_dev_r8_at

      subroutine rrtmg_lw_cloud_cover_dev_r4_at &
            (ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, cldtot, cldcum, cldlay, submask, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      real(kind=r4), target :: play, cldfr
      real(kind=r4), target, optional :: alpha, cldtot, cldcum, cldlay
      integer(c_int32_t), target, optional :: submask
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(5)

      p = c_null_ptr
      if (present(alpha)) p(1) = c_loc(alpha)
      if (present(cldtot)) p(2) = c_loc(cldtot)
      if (present(cldcum)) p(3) = c_loc(cldcum)
      if (present(cldlay)) p(4) = c_loc(cldlay)
      if (present(submask)) p(5) = c_loc(submask)
      call dev_cover(4, ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, c_loc(play), c_loc(cldfr), p, stream)

      end subroutine rrtmg_lw_cloud_cover_dev_r4_at

      subroutine rrtmg_lw_cloud_optics_dev_r8 &
            (ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr, &
             taucloud, ncbands, secdiff, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw
      real(kind=rb), target :: cldfr(ld,*), taucld(16,ld,*), cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*)
      real(kind=rb), target, optional :: plev(ld,*), h2ovmr(ld,*), taucloud(ld,nlay,*), secdiff(ld,*)
      integer(c_int32_t), target, optional :: ncbands(*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(11)

      p = c_null_ptr
      p(1) = c_loc(cldfr); p(2) = c_loc(taucld); p(3) = c_loc(cicewp); p(4) = c_loc(cliqwp); p(5) = c_loc(reice); p(6) = c_loc(reliq)
      if (present(plev)) p(7) = c_loc(plev)
      if (present(h2ovmr)) p(8) = c_loc(h2ovmr)
      if (present(taucloud)) p(9) = c_loc(taucloud)
      if (present(ncbands)) p(10) = c_loc(ncbands)
      if (present(secdiff)) p(11) = c_loc(secdiff)
      call dev_cloud_optics(8, ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, p, stream)

      end subroutine rrtmg_lw_cloud_optics_dev_r8

      subroutine rrtmg_lw_cloud_optics_dev_r4 &
            (ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr, &
             taucloud, ncbands, secdiff, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw
      real(kind=r4), target :: cldfr(ld,*), taucld(16,ld,*), cicewp(ld,*), cliqwp(ld,*), reice(ld,*), reliq(ld,*)
      real(kind=r4), target, optional :: plev(ld,*), h2ovmr(ld,*), taucloud(ld,nlay,*), secdiff(ld,*)
      integer(c_int32_t), target, optional :: ncbands(*)
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(11)

      p = c_null_ptr
      p(1) = c_loc(cldfr); p(2) = c_loc(taucld); p(3) = c_loc(cicewp); p(4) = c_loc(cliqwp); p(5) = c_loc(reice); p(6) = c_loc(reliq)
      if (present(plev)) p(7) = c_loc(plev)
      if (present(h2ovmr)) p(8) = c_loc(h2ovmr)
      if (present(taucloud)) p(9) = c_loc(taucloud)
      if (present(ncbands)) p(10) = c_loc(ncbands)
      if (present(secdiff)) p(11) = c_loc(secdiff)
      call dev_cloud_optics(4, ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, p, stream)

      end subroutine rrtmg_lw_cloud_optics_dev_r4

      subroutine rrtmg_lw_cloud_optics_dev_r8_at &
            (ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr, &
             taucloud, ncbands, secdiff, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw
      real(kind=rb), target :: cldfr, taucld, cicewp, cliqwp, reice, reliq
      real(kind=rb), target, optional :: plev, h2ovmr, taucloud, secdiff
      integer(c_int32_t), target, optional :: ncbands
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(11)

      p = c_null_ptr
      p(1) = c_loc(cldfr); p(2) = c_loc(taucld); p(3) = c_loc(cicewp); p(4) = c_loc(cliqwp); p(5) = c_loc(reice); p(6) = c_loc(reliq)
      if (present(plev)) p(7) = c_loc(plev)
      if (present(h2ovmr)) p(8) = c_loc(h2ovmr)
      if (present(taucloud)) p(9) = c_loc(taucloud)
      if (present(ncbands)) p(10) = c_loc(ncbands)
      if (present(secdiff)) p(11) = c_loc(secdiff)
      call dev_cloud_optics(8, ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, p, stream)

      end subroutine rrtmg_lw_cloud_optics_dev_r8_at

      subroutine rrtmg_lw_cloud_optics_dev_r4_at &
            (ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr, &
             taucloud, ncbands, secdiff, stream)

      integer(kind=im), intent(in) :: ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw
      real(kind=r4), target :: cldfr, taucld, cicewp, cliqwp, reice, reliq
      real(kind=r4), target, optional :: plev, h2ovmr, taucloud, secdiff
      integer(c_int32_t), target, optional :: ncbands
      type(c_ptr), intent(in), optional :: stream

      type(c_ptr) :: p(11)

      p = c_null_ptr
      p(1) = c_loc(cldfr); p(2) = c_loc(taucld); p(3) = c_loc(cicewp); p(4) = c_loc(cliqwp); p(5) = c_loc(reice); p(6) = c_loc(reliq)
      if (present(plev)) p(7) = c_loc(plev)
      if (present(h2ovmr)) p(8) = c_loc(h2ovmr)
      if (present(taucloud)) p(9) = c_loc(taucloud)
      if (present(ncbands)) p(10) = c_loc(ncbands)
      if (present(secdiff)) p(11) = c_loc(secdiff)
      call dev_cloud_optics(4, ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, p, stream)

      end subroutine rrtmg_lw_cloud_optics_dev_r4_at

      ! ... of rrtmg_lw_cloud_optics_dev: p in the C entry's order (the six cloud arrays, plev, h2ovmr, taucloud, ncbands, secdiff; null where absent)
      subroutine dev_cloud_optics(real_bytes, ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw, p, stream)
      integer, intent(in) :: real_bytes
      integer(kind=im), intent(in) :: ncol, ld, nlay, imca, inflglw, iceflglw, liqflglw
      type(c_ptr), intent(in) :: p(11)
      type(c_ptr), intent(in), optional :: stream

      type(array_view) :: view
      type(c_ptr) :: s
      integer(c_int) :: rc

      view = array_view(int(real_bytes, c_int), 0_c_int, 0_c_int, int(ld, c_int))
      s = c_null_ptr
      if (present(stream)) s = stream
      rc = rrtmg_lw_hip_cloud_optics_device_view(view, int(ncol, c_int), int(nlay, c_int), int(imca, c_int), int(inflglw, c_int), &
            int(iceflglw, c_int), int(liqflglw, c_int), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8), p(9), p(10), p(11), s)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_cloud_optics_dev')
      end subroutine dev_cloud_optics

      ! what every specific of rrtmg_lw_dev / rrtmg_lw_mcica_dev ends in: the addresses in the C entry's order - pin: the 23 input arrays
      ! of rrtmg_lw, then alpha; pout: the eight broadband outputs, then the spectral four (null where absent)
      subroutine dev_solve(who, real_bytes, mcica, ncol, ld, nlay, icld, idrv, permuteseed, irng, inflglw, iceflglw, liqflglw, pin, pout, stream)
      character(len=*), intent(in) :: who
      integer, intent(in) :: real_bytes
      logical, intent(in) :: mcica
      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(c_int), intent(in) :: permuteseed
      integer(c_int), intent(inout) :: irng
      type(c_ptr), intent(in) :: pin(24), pout(12)
      type(c_ptr), intent(in), optional :: stream

      type(array_view) :: view
      type(c_ptr) :: s
      integer(c_int) :: rc, icld_c

      view = array_view(int(real_bytes, c_int), 0_c_int, 0_c_int, int(ld, c_int))
      s = c_null_ptr
      if (present(stream)) s = stream
      icld_c = int(icld, c_int)
      if (mcica) then
         rc = rrtmg_lw_hip_run_mcica_subcol_device_view(view, int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), permuteseed, irng, &
               pin(1), pin(2), pin(3), pin(4), pin(5), pin(6), pin(7), pin(8), pin(9), pin(10), pin(11), pin(12), pin(13), pin(14), pin(15), &
               pin(16), int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), pin(17), pin(18), pin(19), pin(20), pin(21), pin(22), &
               pin(24), pin(23), pout(1), pout(2), pout(3), pout(4), pout(5), pout(6), pout(7), pout(8), pout(9), pout(10), pout(11), pout(12), s)
      else
         rc = rrtmg_lw_hip_run_nomcica_device_view(view, int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), &
               pin(1), pin(2), pin(3), pin(4), pin(5), pin(6), pin(7), pin(8), pin(9), pin(10), pin(11), pin(12), pin(13), pin(14), pin(15), &
               pin(16), int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), pin(17), pin(18), pin(19), pin(20), pin(21), pin(22), &
               pin(23), pout(1), pout(2), pout(3), pout(4), pout(5), pout(6), pout(7), pout(8), pout(9), pout(10), pout(11), pout(12), s)
      endif
      if (rc /= 0) call rrtmg_lw_hip_abort(who)
      icld = int(icld_c, im)
      end subroutine dev_solve

      ! ... of rrtmg_lw_mcica_samples_dev: pin as above; pout: the eight broadband outputs, then uflx_var, dflx_var, hr_var
      subroutine dev_samples(real_bytes, ncol, ld, nlay, icld, idrv, permuteseed, nsamp, seedstep, irng, inflglw, iceflglw, liqflglw, pin, pout, stream)
      integer, intent(in) :: real_bytes
      integer(kind=im), intent(in) :: ncol, ld, nlay, idrv, inflglw, iceflglw, liqflglw
      integer(kind=im), intent(inout) :: icld
      integer(c_int), intent(in) :: permuteseed, nsamp, seedstep
      integer(c_int), intent(inout) :: irng
      type(c_ptr), intent(in) :: pin(24), pout(11)
      type(c_ptr), intent(in), optional :: stream

      type(array_view) :: view
      type(c_ptr) :: s
      integer(c_int) :: rc, icld_c

      view = array_view(int(real_bytes, c_int), 0_c_int, 0_c_int, int(ld, c_int))
      s = c_null_ptr
      if (present(stream)) s = stream
      icld_c = int(icld, c_int)
      rc = rrtmg_lw_hip_run_mcica_samples_device_view(view, int(ncol, c_int), int(nlay, c_int), icld_c, int(idrv, c_int), permuteseed, nsamp, &
            seedstep, irng, &
            pin(1), pin(2), pin(3), pin(4), pin(5), pin(6), pin(7), pin(8), pin(9), pin(10), pin(11), pin(12), pin(13), pin(14), pin(15), &
            pin(16), int(inflglw, c_int), int(iceflglw, c_int), int(liqflglw, c_int), pin(17), pin(18), pin(19), pin(20), pin(21), pin(22), &
            pin(24), pin(23), pout(1), pout(2), pout(3), pout(4), pout(5), pout(6), pout(7), pout(8), pout(9), pout(10), pout(11), s)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_mcica_samples_dev')
      icld = int(icld_c, im)
      end subroutine dev_samples

      ! ... of rrtmg_lw_alpha_dev
      subroutine dev_alpha(real_bytes, ncol, ld, nlay, icld, idcor, decorr_con, dz, lat, juldat, cldfrac, alpha, stream)
      integer, intent(in) :: real_bytes
      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, idcor, juldat
      real(c_double), intent(in) :: decorr_con
      type(c_ptr), intent(in) :: dz, lat, cldfrac, alpha
      type(c_ptr), intent(in), optional :: stream

      type(array_view) :: view
      type(c_ptr) :: s
      integer(c_int) :: rc

      view = array_view(int(real_bytes, c_int), 0_c_int, 0_c_int, int(ld, c_int))
      s = c_null_ptr
      if (present(stream)) s = stream
      rc = rrtmg_lw_hip_get_alpha_device_view(view, int(ncol, c_int), int(nlay, c_int), int(icld, c_int), int(idcor, c_int), decorr_con, &
            dz, lat, int(juldat, c_int), cldfrac, alpha, s)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_alpha_dev')
      end subroutine dev_alpha

      ! ... of rrtmg_lw_cloud_cover_dev: p = alpha, cldtot, cldcum, cldlay, submask (null where absent)
      subroutine dev_cover(real_bytes, ncol, ld, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, p, stream)
      integer, intent(in) :: real_bytes
      integer(kind=im), intent(in) :: ncol, ld, nlay, icld, permuteseed, nsamp, seedstep
      integer(kind=im), intent(inout) :: irng
      type(c_ptr), intent(in) :: play, cldfr, p(5)
      type(c_ptr), intent(in), optional :: stream

      type(array_view) :: view
      type(c_ptr) :: s
      integer(c_int) :: rc, irng_c

      view = array_view(int(real_bytes, c_int), 0_c_int, 0_c_int, int(ld, c_int))
      s = c_null_ptr
      if (present(stream)) s = stream
      irng_c = int(irng, c_int)
      rc = rrtmg_lw_hip_mcica_cloud_cover_device_view(view, int(ncol, c_int), int(nlay, c_int), int(icld, c_int), int(permuteseed, c_int), &
            int(nsamp, c_int), int(seedstep, c_int), irng_c, play, cldfr, p(1), p(2), p(3), p(4), p(5), s)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_cloud_cover_dev')
      irng = int(irng_c, im)
      end subroutine dev_cover

      ! ... and of rrtmg_lw_dtsfc_dev: p in the C entry's order (plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt, the four outputs)
      subroutine dev_adjust(real_bytes, ncol, ld, nlay, p, stream)
      integer, intent(in) :: real_bytes
      integer(kind=im), intent(in) :: ncol, ld, nlay
      type(c_ptr), intent(in) :: p(12)
      type(c_ptr), intent(in), optional :: stream

      type(array_view) :: view
      type(c_ptr) :: s
      integer(c_int) :: rc

      view = array_view(int(real_bytes, c_int), 0_c_int, 0_c_int, int(ld, c_int))
      s = c_null_ptr
      if (present(stream)) s = stream
      rc = rrtmg_lw_hip_adjust_tsfc_device_view(view, int(ncol, c_int), int(nlay, c_int), p(1), p(2), p(3), p(4), p(5), p(6), p(7), p(8), &
            p(9), p(10), p(11), p(12), s)
      if (rc /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_dtsfc_dev')
      end subroutine dev_adjust

      ! Waits for `stream` (absent: the default stream) and reports what the calls enqueued on it have found: the code of
      ! rrtmg_lw_hip_check, 0 when all is well
      function rrtmg_lw_dev_status(stream) result(rc)
      type(c_ptr), intent(in), optional :: stream
      integer :: rc
      type(c_ptr) :: s
      s = c_null_ptr
      if (present(stream)) s = stream
      rc = int(rrtmg_lw_hip_check(s))
      end function rrtmg_lw_dev_status

      ! ... or ends as the host shims end: the library's text, error stop
      subroutine rrtmg_lw_dev_check(stream)
      type(c_ptr), intent(in), optional :: stream
      if (rrtmg_lw_dev_status(stream) /= 0) call rrtmg_lw_hip_abort('rrtmg_lw_dev_check')
      end subroutine rrtmg_lw_dev_check

      end module rrtmg_lw_device
