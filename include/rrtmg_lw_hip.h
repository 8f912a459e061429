/*
 * rrtmg_lw_hip.h - C ABI of the MI355X-native RRTMG_LW column solver (librrtmg_lw_hip.so).
 *
 * Drop-in boundary for the reference's GCM entry points.  A host model keeps calling
 *     use rrtmg_lw_init, only: rrtmg_lw_ini      (reference: src/rrtmg_lw_init.f90:47)
 *     use rrtmg_lw_rad,  only: rrtmg_lw          (reference: src/rrtmg_lw_rad.nomcica.f90:99-108,
 *                                                 McICA flavour src/rrtmg_lw_rad.f90:99-108)
 * through the ISO_C_BINDING shim modules shipped in rrtmg_lw_amd/fortran/, which forward to the
 * functions below.  Plain pointers and sizes only; every array is float64 in Fortran (column-major)
 * order exactly as the reference declares it:
 *     play,tlay,*vmr,cldfr,cicewp,cliqwp,reice,reliq  (ncol,nlay)      plev,tlev  (ncol,nlay+1)
 *     tsfc (ncol)   emis (ncol,16)   taucld (16,ncol,nlay)   tauaer (ncol,nlay,16)
 *     uflx,dflx,uflxc,dflxc,duflx_dt,duflxc_dt (ncol,nlay+1)   hr,hrc (ncol,nlay)
 *     McICA: cldfmcl,taucmcl,ciwpmcl,clwpmcl (140,ncol,nlay)   reicmcl,relqmcl (ncol,nlay)
 * Layer 1 is the surface layer; pressures in hPa.  The caller owns every array.
 *
 * Return value: 0 on success; non-zero = error, text available from rrtmg_lw_hip_last_error()
 * (the reference `stop 'MESSAGE'`s instead - src/rrtmg_lw_cldprop.f90:212,217,228,244,272; the
 * Fortran shim turns a non-zero code into `error stop` with the same text).
 * There is no CPU fallback: every entry fails with RRTMG_LW_HIP_ENODEVICE when no GPU is usable.
 */
#ifndef RRTMG_LW_HIP_H
#define RRTMG_LW_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RRTMG_LW_HIP_OK 0
#define RRTMG_LW_HIP_EPHYSICS 1   /* the reference would `stop` (bad particle size / flag) */
#define RRTMG_LW_HIP_EARG 2
#define RRTMG_LW_HIP_ENODEVICE 3
#define RRTMG_LW_HIP_ENOTINIT 4
#define RRTMG_LW_HIP_EDATA 5      /* table / k-data file missing or malformed */
#define RRTMG_LW_HIP_EHIP 6       /* HIP runtime error */

#define RRTMG_LW_NBND 16
#define RRTMG_LW_NGPT 140

/* rrtmg_lw_ini(cpdair)  -  reference: src/rrtmg_lw_init.f90:47-194.
 * Reads the static tables (lw_static.bin) and the absorption-coefficient file (RRLWBLOB k-data,
 * original 16-g form; see rrtmg_lw_amd/kdata.py for the converters from rrtmg_lw_k_g.f90 and
 * rrtmg_lw.nc), performs the 256->140 g-point reduction and the LUT build on the host, and uploads the
 * packed, g-point-fastest tables to the device `device` (HIP ordinal of this process's GPU).
 * cpdair in J kg-1 K-1 sets heatfac (src/rrtmg_lw_init.f90:298). */
int rrtmg_lw_hip_init(const char *static_tables_path, const char *kdata_path, double cpdair, int device);

/* The same for SEVERAL GPUs driven by one process (SURVEY.md 8b `ndev`; the reference's calling model is one serial `do iplon` loop,
 * src/rrtmg_lw_rad.nomcica.f90:472: a non-MPI host has one process).  devices[0 .. ndev-1] are HIP ordinals; the host-pointer entries
 * rrtmg_lw_hip_run_nomcica and rrtmg_lw_hip_run_mcica then split their columns into ndev contiguous blocks and feed every device from
 * its own host thread (its own PCIe link, copy streams and workspace); every other entry works on devices[0].  An ordinal may be
 * listed more than once ("virtual devices": separate workspaces and streams on one GPU - how the fan-out is tested on a one-GPU box).
 * The Fortran shim calls this from rrtmg_lw_ini when RRTMG_LW_NDEV is set (devices RRTMG_LW_DEVICE, +1, ...; RRTMG_LW_VIRTUAL_DEVICES=1
 * keeps them all on RRTMG_LW_DEVICE). */
int rrtmg_lw_hip_init_devices(const char *static_tables_path, const char *kdata_path, double cpdair, int ndev, const int *devices);
int rrtmg_lw_hip_num_devices(void);     /* 0 before initialisation */

/* 1 if the loaded k-data is the synthetic stand-in (fluxes not physical), 0 if real, -1 if not initialised */
int rrtmg_lw_hip_kdata_is_standin(void);

void rrtmg_lw_hip_finalize(void);
/* Text of the calling THREAD's last error (concurrent callers each read their own); of the library's last one if this thread has had none. */
const char *rrtmg_lw_hip_last_error(void);

/* rrtmg_lw, non-McICA  -  reference: src/rrtmg_lw_rad.nomcica.f90:99-588.  HOST pointers.
 * icld is in/out (reset to 2 when outside [0,3], :456).  duflx_dt/duflxc_dt may be NULL unless idrv==1. */
int rrtmg_lw_hip_run_nomcica(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt);

/* The device-pointer entries below run on the state of the device their arrays live on (hipPointerGetAttributes on `play`): after
 * rrtmg_lw_hip_init_devices a one-process host with device-resident data on several GPUs uses all of them through the same entries;
 * arrays on a device the library was not initialised for are an error.  (The Mersenne-Twister generator, irng = 1 - one stream over all
 * columns of a call - lives on the first device.)  rrtmg_lw_hip_last_device_state: the index of the state this thread's last such call
 * ran on.  rrtmg_lw_hip_check(stream) waits for the stream and reports the first physics error of any state. */
int rrtmg_lw_hip_last_device_state(void);
/* Same contract with DEVICE pointers (a GPU-resident host model, and the benchmark's timed region).
 * Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) and the call
 * returns without synchronising; physics errors are reported by rrtmg_lw_hip_check(stream). */
int rrtmg_lw_hip_run_nomcica_device(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, void *stream);

/* Synchronise `stream` and return the physics-error status of the work enqueued so far. */
int rrtmg_lw_hip_check(void *stream);

/* Prepared-column entry (HOST pointers): the physics sequence of the reference's column driver,
 * cldprop -> setcoef -> taumol -> rtrn|rtrnmr (src/rrtmg_lw.1col.f90:497-580), for `ncol` independent
 * columns that all have `nlayers` layers.  This is the interface the golden OUTPUT_RRTM files pin
 * (column amounts come from the input file, not from inatm's hydrostatic estimate).
 * Arrays are column-fastest: pavel,tavel,coldry,wbrodl,cldfrac,ciwp,clwp,rei,rel (ncol,nlayers);
 * pz,tz (ncol,0:nlayers); tbound,pwvcm (ncol); semiss (ncol,16); wkl (ncol,7,nlayers); wx (ncol,4,nlayers);
 * tauc (ncol,16,nlayers); taua (ncol,nlayers,16); outputs (ncol,0:nlayers).
 * istart..iend select the bands (1..16), any range (the reference's own sweeps support one band, iout > 0, or a range from band 1:
 * with iout = 0 their g-point counter starts at 1 whatever istart is, src/rrtmg_lw_rtrn.f90:354-360); istart==16 switches band 16 to the
 * 2600-3250 cm-1 Planck table
 * exactly as setcoef does (src/rrtmg_lw_setcoef.f90:233-252).  icld==1 -> rtrn, otherwise rtrnmr. */
int rrtmg_lw_hip_run_columns(
    int ncol, int nlayers, int istart, int iend, int icld, int idrv,
    const double *pavel, const double *tavel, const double *pz, const double *tz, const double *tbound,
    const double *semiss, const double *coldry, const double *wkl, const double *wbrodl, const double *wx,
    const double *pwvcm, int inflag, int iceflag, int liqflag, const double *cldfrac, const double *tauc,
    const double *ciwp, const double *clwp, const double *rei, const double *rel, const double *taua,
    double *totuflux, double *totdflux, double *fnet, double *htr,
    double *totuclfl, double *totdclfl, double *fnetc, double *htrc,
    double *dtotuflux_dt, double *dtotuclfl_dt);

/* McICA flavour of the prepared-column entry (HOST pointers): one Monte-Carlo sample of the column driver with imca = 1,
 * cldprmc -> setcoef -> taumol -> rtrnmc (src/rrtmg_lw.1col.f90:471-580), for `ncol` (column, sample) pairs.  Arrays as for
 * rrtmg_lw_hip_run_columns, the cloud arguments replaced by the sub-columns cldfmc, taucmc, ciwpmc, clwpmc (140,ncol,nlayers)
 * and reicmc, relqmc (ncol,nlayers).  The driver's result is the mean over its nmca = 200 samples, sample `ims` being generated
 * with permuteseed = ims * 140 (src/mcica_subcol_gen_lw.1col.f90:248-251). */
int rrtmg_lw_hip_run_columns_mcica(
    int ncol, int nlayers, int istart, int iend, int icld, int idrv,
    const double *pavel, const double *tavel, const double *pz, const double *tz, const double *tbound,
    const double *semiss, const double *coldry, const double *wkl, const double *wbrodl, const double *wx,
    const double *pwvcm, int inflag, int iceflag, int liqflag, const double *cldfmc, const double *taucmc,
    const double *ciwpmc, const double *clwpmc, const double *reicmc, const double *relqmc, const double *taua,
    double *totuflux, double *totdflux, double *fnet, double *htr,
    double *totuclfl, double *totdclfl, double *fnetc, double *htrc,
    double *dtotuflux_dt, double *dtotuclfl_dt);

/* McICA flavour ---------------------------------------------------------------------------------- */
/* rrtmg_lw, McICA  -  reference: src/rrtmg_lw_rad.f90:99-594 (cldprmc src/rrtmg_lw_cldprmc.f90:49, rtrnmc
 * src/rrtmg_lw_rtrnmc.f90:51).  HOST pointers; same contract as rrtmg_lw_hip_run_nomcica with the cloud
 * arguments replaced by the sub-column arrays cldfmcl,taucmcl,ciwpmcl,clwpmcl (140,ncol,nlay) and
 * reicmcl,relqmcl (ncol,nlay).  icld is reset to 2 when outside [0,3] (:469); icld==0 ignores the cloud arrays. */
int rrtmg_lw_hip_run_mcica(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfmcl, const double *taucmcl, const double *ciwpmcl, const double *clwpmcl,
    const double *reicmcl, const double *relqmcl, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt);

/* DEVICE-pointer variant (enqueue on `stream`, no synchronisation; see rrtmg_lw_hip_check). */
int rrtmg_lw_hip_run_mcica_device(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfmcl, const double *taucmcl, const double *ciwpmcl, const double *clwpmcl,
    const double *reicmcl, const double *relqmcl, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, void *stream);

/* get_alpha  -  reference: src/mcica_subcol_gen_lw.f90:68-180.  HOST pointers; dz,cldfrac,alpha (ncol,nlay),
 * lat (ncol).  alpha is written only for icld = 4 or 5 (exponential / exponential-random overlap). */
int rrtmg_lw_hip_get_alpha(int ncol, int nlay, int icld, int idcor, double decorr_con, const double *dz, const double *lat,
                           int juldat, const double *cldfrac, double *alpha);

/* mcica_subcol_lw  -  reference: src/mcica_subcol_gen_lw.f90:183-291 (generate_stochastic_clouds :295-703,
 * kissvec :711-745, Mersenne Twister src/mcica_random_numbers.f90).  HOST pointers.
 * play,cldfrac,ciwp,clwp,rei,rel,alpha (ncol,nlay); tauc (16,ncol,nlay); outputs cldfmcl,ciwpmcl,clwpmcl,taucmcl
 * (140,ncol,nlay), reicmcl,relqmcl (ncol,nlay).  icld 1..5 = random, maximum-random, maximum, exponential,
 * exponential-random overlap (alpha may be NULL unless icld is 4 or 5); icld 0 returns without touching the
 * outputs.  irng is in/out (any non-zero value becomes 1): 0 = kissvec, one stream per column seeded from
 * its four lowest layer pressures; 1 = one Mersenne-Twister stream seeded with permuteseed, consumed in
 * (sub-column, column, layer) order.  kissvec: 4 <= nlay <= 603 (modules/parrrtm.f90:31; the column driver's mxlay is 203); a permuteseed the library
 * has not seen builds a small jump-ahead table on the host; the tables of the last 128 seeds are kept. */
int rrtmg_lw_hip_mcica_subcol(
    int ncol, int nlay, int icld, int permuteseed, int *irng, const double *play, const double *cldfrac, const double *ciwp,
    const double *clwp, const double *rei, const double *rel, const double *tauc, const double *alpha,
    double *cldfmcl, double *ciwpmcl, double *clwpmcl, double *reicmcl, double *relqmcl, double *taucmcl);

/* DEVICE-pointer variant (enqueue on `stream`; the irng = 1 stream is drawn on the device as well: chunk-parallel by jump-ahead of
 * MT19937, the chunk states cached per (permuteseed, ncol * nlay), a new seed costs one device synchronisation and 10-30 ms). */
int rrtmg_lw_hip_mcica_subcol_device(
    int ncol, int nlay, int icld, int permuteseed, int *irng, const double *play, const double *cldfrac, const double *ciwp,
    const double *clwp, const double *rei, const double *rel, const double *tauc, const double *alpha,
    double *cldfmcl, double *ciwpmcl, double *clwpmcl, double *reicmcl, double *relqmcl, double *taucmcl, void *stream);

/* mcica_subcol_lw + McICA rrtmg_lw in one call (the sequence a host model runs every radiation step,
 * README.md / src/rrtmg_lw_rad.f90:140-150), without materialising the (140,ncol,nlay) arrays: the generator
 * leaves a 140-bit cloud mask per (column, layer) on the device and cldprmc/rtrnmc consume it directly.
 * Results equal rrtmg_lw_hip_mcica_subcol followed by rrtmg_lw_hip_run_mcica.  Cloud arguments are the
 * generator's inputs (cldfr,cicewp,cliqwp,reice,reliq,alpha (ncol,nlay); taucld (16,ncol,nlay)); icld in
 * [0,5] selects the overlap for the generator and comes back as rrtmg_lw would leave it. */
int rrtmg_lw_hip_run_mcica_subcol(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *alpha, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt);

int rrtmg_lw_hip_run_mcica_subcol_device(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *alpha, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, void *stream);

/* The mean over several sub-column samples ---------------------------------------------------------- */
/* One call of the fused entry returns the fluxes of ONE set of sub-columns; the reference's column driver averages 200 of them
 * (src/rrtmg_lw.1col.f90:457-480, :641-660).  These two entries do that at GCM width.  Their argument lists are those of
 * rrtmg_lw_hip_run_mcica_subcol / _device with `nsamp, seedstep` behind permuteseed.  With X_s what that entry returns in output X when
 * called with permuteseed + s * seedstep, s = 0 .. nsamp-1:
 *     uflx, dflx, hr, duflx_dt       (((X_0 + X_1) + X_2) + ... + X_{nsamp-1}) / nsamp: the float64 sum in sample order, then ONE IEEE
 *                                    division (not a multiplication by a reciprocal) - bit for bit what a caller gets who runs the
 *                                    nsamp calls and averages in that order
 *     uflxc, dflxc, hrc, duflxc_dt   X_0 itself: the clear-sky stream does not depend on the sample and is written once
 * seedstep: the generator skips `permuteseed` draws of every column's stream (src/mcica_subcol_gen_lw.f90:472-474) and asks callers to
 * offset seeds by the number of sub-columns (:193-196, :262), so rrtmg_lw_hip_gpoints() - 140, 256 in the g256 build - is the documented
 * choice.  nsamp = 1 is rrtmg_lw_hip_run_mcica_subcol[_device]; *icld = 0 draws nothing and returns that single call's outputs whatever
 * nsamp is.  icld is in/out and reset as the fused entry does it; optional outputs keep its NULL rules (duflx_dt, duflxc_dt with idrv = 1).
 * RRTMG_LW_HIP_EARG, with a text that names the argument and before any output is written: nsamp < 1, nsamp > RRTMG_LW_HIP_MAX_SAMPLES,
 * seedstep < 1, permuteseed + (nsamp-1) * seedstep not an int, *irng != 0 together with nsamp > 1 (the Mersenne-Twister stream is out of
 * scope: its chunk-state cache holds two seeds).  A physics error in any sample is reported as the single call reports it - by the
 * device entry through rrtmg_lw_hip_check(stream).
 * The device entry enqueues on `stream` and does not synchronise; in steady state - the same (permuteseed, seedstep, nsamp, nlay, icld)
 * as an earlier call since initialisation - that includes the generator's jump tables, which are kept per (draws per sub-column, seed)
 * in a set of 128 - larger than RRTMG_LW_HIP_MAX_SAMPLES - so that a single-seed call between two averaging calls rebuilds nothing either;
 * once 128 pairs have been seen a new one replaces the pair used longest ago, after one device synchronisation
 * (rrtmg_lw_hip_kiss_tables_built counts the tables built).  It never reads the output arrays before it has written them.  The host
 * entry takes the entry lock like any other call, does not join the combining of concurrent small calls, and keeps the whole call's
 * arrays on the device while it runs (the samples add up there): about 0.5 KB per column and layer beside the workspace, allocated
 * for the call and not counted by rrtmg_lw_hip_workspace_bytes - a call too large for that is made in column blocks by the caller.
 * What the samples share: the argument checks, the workspace, the jump tables, the clear-sky outputs (stored by sample 0 only), the
 * averaging, which k_flux does as it stores (sample 0 stores, the others add, the last one adds and divides: no pass over the outputs
 * of its own), and the gas optics: per batch of columns k_layer runs once, with the first sample, and leaves the cells' float64 optical
 * depths in the workspace; the total codes of a later sample's cloudy layers are formed from them by a small kernel (k_codet) with
 * k_layer's expressions.  The workspace holds those optical depths in the arrays the McICA entry with sub-column arrays uses (1.2 KB per
 * column and layer, and as much again for that entry's emissivity array, which comes with it: the workspace of a call of that entry).  Every sample still runs the per-column kernels, the generator, the
 * cloud optics and all sweeps, the clear-sky ones included.
 * nsamp = 1 and *icld = 0 through the host entry ARE rrtmg_lw_hip_run_mcica_subcol behind the entry lock - its fan-out over several
 * initialised devices included; with nsamp > 1 and cloud the host entry runs on the first device.
 * The sample variance (rrtmg_lw_hip_run_mcica_samples_var, rrtmg_lw_hip_run_mcica_samples_device_view): three optional outputs uflx_var,
 * dflx_var, hr_var with the shapes of uflx, dflx, hr, each NULL or set on its own.  They hold the UNBIASED sample variance of the nsamp
 * values X_s, in (W m-2)^2 and (K d-1)^2; the standard error of the returned mean is sqrt(var / nsamp) - what tells a host whether
 * nsamp = 4 or 16 is enough.  It is formed where the mean is formed, per output element, in float64, every operation rounded on its own
 * (no fused multiply-add), with S in the mean's array and M in the variance's - no third array, no pass of its own, no workspace:
 *     sample 0:                       S = X_0                       M = 0
 *     sample s >= 1, c = s + 1:       S = S + X_s
 *                                     t = c * X_s - S               (the product rounds, then the difference)
 *                                     M = M + (t * t) / (c * (c - 1))          (c * (c - 1) is exact)
 *     last sample, after its update:  mean = S / nsamp              var = M / (nsamp - 1)
 * so a caller who runs the nsamp single calls and applies these lines gets the same bits, and the mean is bit for bit that of the entries
 * without variance.  var >= 0 by construction; columns whose samples are identical (no cloud) give exactly 0 or values at rounding
 * level (below (nsamp x 2^-53)^2: a few 1e-25 for fluxes of 50 - 500 W m-2 and 64 samples).  When nothing is drawn (*icld = 0) the variance arrays are written with exact
 * zeros - by the kernel that stores the fluxes, so a view is not written outside the call's columns.  The clear-sky outputs and duflx_dt
 * get no variance.  RRTMG_LW_HIP_EARG before any output is written, with a text that names the argument: a variance pointer together
 * with nsamp = 1; a variance array that overlaps its mean.
 * Not offered: *_r4 and *_spectral variants, fan-out over several devices, per-sample outputs, the Mersenne Twister with nsamp > 1. */
#define RRTMG_LW_HIP_MAX_SAMPLES 64
int rrtmg_lw_hip_run_mcica_samples(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int nsamp, int seedstep, int *irng,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *alpha, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt);
int rrtmg_lw_hip_run_mcica_samples_device(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int nsamp, int seedstep, int *irng,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *alpha, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, void *stream);
/* HOST pointers: rrtmg_lw_hip_run_mcica_samples plus the variances; the three arrays join the per-call allocation on the device.  With
 * a variance pointer set, *icld = 0 runs on the first device too. */
int rrtmg_lw_hip_run_mcica_samples_var(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int nsamp, int seedstep, int *irng,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *alpha, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, double *uflx_var, double *dflx_var, double *hr_var);
/* jump tables of the kissvec generator built since the library was loaded (a counter, like rrtmg_lw_hip_graph_stats) */
long long rrtmg_lw_hip_kiss_tables_built(void);

/* Spectral (per-band) fluxes --------------------------------------------------------------------- */
/* The six entries below take the argument list of the entry they are named after, followed by four more outputs (in the device entries
 * in front of `stream`), and compute everything that entry computes - the broadband outputs bit for bit as it does - plus, per band:
 *     uflxs, dflxs      total-sky upward / downward flux of each band     (ncol,nlay+1,16), required
 *     uflxcs, dflxcs    clear-sky upward / downward flux of each band     (ncol,nlay+1,16), both NULL or both set
 * Element (i, k, b), 0-based, lies at i + ncol*(k + (nlay+1)*b): columns fastest, level 0 at the surface, band last (a host that keeps
 * band-first arrays, as CAM does, transposes).  The flux of band b at level k is the term the reference adds into totuflux(k) /
 * totdflux(k) / totuclfl(k) / totdclfl(k) for that band, uflux(k) x delwave(b) x fluxfac (src/rrtmg_lw_rtrn.f90:549-562 and the same
 * lines of rtrnmr / rtrnmc); summed over the 16 bands it gives uflx / dflx / uflxc / dflxc up to rounding.
 * Band 16 is the band's share of a broadband call: its Planck function runs from 2600 cm-1 to infinity (src/rrtmg_lw_setcoef.f90:228-252).
 * It is NOT the column driver's IOUT = 16 / 99 output, which uses the 2600-3250 cm-1 table (rrtmg_lw_hip_run_columns with istart = 16).
 * Heating rates and d(flux)/dT stay broadband (duflx_dt / duflxc_dt as in the plain entries).  The host-pointer spectral entries do not
 * join the combining of concurrent small calls: they take the library's entry lock like any other call.  A NULL uflxs or dflxs, or only
 * one of uflxcs / dflxcs, is RRTMG_LW_HIP_EARG. */
int rrtmg_lw_hip_run_nomcica_spectral(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, double *uflxs, double *dflxs, double *uflxcs, double *dflxcs);
int rrtmg_lw_hip_run_nomcica_spectral_device(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, double *uflxs, double *dflxs, double *uflxcs, double *dflxcs, void *stream);
int rrtmg_lw_hip_run_mcica_spectral(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfmcl, const double *taucmcl, const double *ciwpmcl, const double *clwpmcl,
    const double *reicmcl, const double *relqmcl, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, double *uflxs, double *dflxs, double *uflxcs, double *dflxcs);
int rrtmg_lw_hip_run_mcica_spectral_device(
    int ncol, int nlay, int *icld, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfmcl, const double *taucmcl, const double *ciwpmcl, const double *clwpmcl,
    const double *reicmcl, const double *relqmcl, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, double *uflxs, double *dflxs, double *uflxcs, double *dflxcs, void *stream);
int rrtmg_lw_hip_run_mcica_subcol_spectral(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *alpha, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, double *uflxs, double *dflxs, double *uflxcs, double *dflxcs);
int rrtmg_lw_hip_run_mcica_subcol_spectral_device(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *alpha, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, double *uflxs, double *dflxs, double *uflxcs, double *dflxcs, void *stream);

/* Tuning / introspection ------------------------------------------------------------------------- */
/* Aggregation of small calls.  A host model that calls rrtmg_lw per chunk of a few dozen columns (the reference is called that way:
 * `do iplon = 1, ncol` inside, pcols-sized chunks outside, src/rrtmg_lw_rad.nomcica.f90:472) pays ~0.5 ms of launch latency per call on
 * the GPU whatever the chunk size.  queue_begin fixes what the chunks share (layer count, flags); queue_add takes one chunk with
 * exactly the argument list of rrtmg_lw_hip_run_nomcica - it only records the pointers, the arrays must stay valid and unchanged until
 * the flush; queue_flush packs all queued chunks column-wise into one pinned staging set, runs ONE pass over all their columns and
 * writes every chunk's outputs (and its icld, reset as rrtmg_lw resets it) back.  Errors of the pass are reported by the flush. */
int rrtmg_lw_hip_queue_begin(int nlay, int icld, int idrv, int inflglw, int iceflglw, int liqflglw);
int rrtmg_lw_hip_queue_add(
    int ncol, int *icld,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *tauaer,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt);
int rrtmg_lw_hip_queue_flush(void);
/* columns queued since the last flush */
int rrtmg_lw_hip_queue_columns(void);

/* What the library was built with: 0 for the shipped library, 8 for the 256-g-point one.  Bit 0: tuning build (-DRRLW_TUNE: only the
 * benchmark's kernels), bit 3: -DRRLW_G256, bit 4: kernel-geometry switches (same results, other speed).  Bits 1 and 2 (knock-out
 * switch, numerics variant) are reserved: these sources no longer set them - the switches behind them are retired, and no build of
 * these sources computes anything but the product's results. */
unsigned rrtmg_lw_hip_build_flags(void);
/* Columns processed per internal batch (bounds the device workspace); 0 = back to the default, which follows the call's layers: 262144 at up
 * to 96 layers, 131072 at 137 (the next lower power of two of 262144 x 72 / nlay) - the benchmark's call (1e6 x 72 layers, rtrnmr) then holds
 * 36.9 GB of workspace, the 137-layer call with aerosol and d/dT 38.7 GB; set_batch(65536) brings the 72-layer call to 9.3 GB at 4 % of its
 * speed (profiles/round5_batch_sweep.md) (0.06-0.16 MB of device workspace per column at 72 layers, by call shape: see rrtmg_lw_hip_workspace_bytes). */
int rrtmg_lw_hip_set_batch(int ncol_batch);
/* The columns per internal batch in force for a call of `nlay` layers: the default by the call's layers, or the size named with
 * rrtmg_lw_hip_set_batch - either one halved until the last row of the largest array the sweeps read by row offset (rtrnmr's overlap
 * factors, (nlay + 1) x 48 bytes per column) ends inside the 0x7ffffff0 bytes their buffer descriptors span: 262144 columns up to 169
 * layers, 131072 up to 340, 65536 up to 681. */
int rrtmg_lw_hip_effective_batch(int nlay);
/* on = 1: device-pointer entries run the sweeps / k_flux of column batch i on a second stream while k_layer of batch i+1 runs on the
 * caller's stream (second scratch set, +0.1 MB of workspace per column).  Default 0: a sweep workgroup owns a CU (transmittance table in
 * LDS, all vector registers), so the two do not share one (measured: 1-2 % faster on 1e6 cloudy columns).  on = 0 frees the second set at the next workspace
 * allocation. */
int rrtmg_lw_hip_set_overlap(int on);
/* CU partition of that overlap: k_layer of batch i+1 runs on `layer_cus` of the device's compute units (rounded to a multiple of 8, the
 * same number from every XCD: hipExtStreamCreateWithCUMask), the sweeps and k_flux of batch i on the others; the first batch's k_layer and
 * the last batch's sweeps, which have nothing beside them, take the whole chip.  layer_cus > 0 switches the overlap on; 0 removes the
 * partition.  Results do not depend on it.  rrtmg_lw_hip_cu_partition() returns the CUs of k_layer's share (0: none). */
int rrtmg_lw_hip_set_cu_partition(int layer_cus);
int rrtmg_lw_hip_cu_partition(void);
/* A cloudy batch too small to fill the chip is a latency chain of kernels, three of them sweeps (down above the clouds, the cloud zone, up
 * above the clouds).  Batches of up to `ncol` columns (default 4096; RRTMG_LW_ONE_SWEEP_MAX) take ONE sweep launch per band group instead:
 * the cloud-zone kernel walks all levels.  0 = never.  Results do not depend on it (bit for bit).  Returns the previous value. */
int rrtmg_lw_hip_set_one_sweep_max(int ncol);
/* ... and its sweeps put twelve waves on each of a few CUs: 1 024 columns are 16 blocks of 64, i.e. 16 workgroups per group of bands.
 * Batches of up to `ncol` columns (default 768: sixteen bands x twelve blocks still find a CU each; RRTMG_LW_SPLIT_MAX) are swept ONE band
 * per workgroup instead - one to four waves - and leave a flux partial per band; k_flux adds the bands of a group first, in the order the group's workgroup adds them,
 * so the results do not depend on it (bit for bit).  0 = never.  Returns the previous value. */
int rrtmg_lw_hip_set_split_max(int ncol);
/* A device-resident call of one batch that does not fill the chip is a chain of a dozen dependent launches on four streams.  The second
 * call with the same arguments (shape, flags, every array pointer - a host model hands over the same arrays step after step) is
 * captured as a graph, later ones are ONE hipGraphLaunch on the caller's stream (up to 8 graphs are kept).  Calls of up to `ncol`
 * columns are taken this way (default 16384; RRTMG_LW_GRAPH_MAX; 0 = never).  Results do not depend on it (bit for bit).  Returns the
 * previous value.  rrtmg_lw_hip_graph_stats: graphs captured / calls replayed since initialisation. */
int rrtmg_lw_hip_set_graph_max(int ncol);
void rrtmg_lw_hip_graph_stats(long long *captures, long long *replays);
/* k_layer stages, per workgroup of 256 columns of one layer, the reference-pressure planes of the absorption tables those columns
 * need.  Where the columns of a model level lie within one plane of each other (a grid that is nearly the same in every column) three
 * planes do; on a terrain-following grid (surface pressures of 550 .. 1040 hPa side by side: up to three planes apart,
 * reference src/rrtmg_lw_setcoef.f90:276-284) such workgroups are taken by a second launch that stages five planes and ten minor-gas
 * temperature slices (GCM entries; default on, RRTMG_LW_WIDE_WINDOW=0 to switch off: every workgroup then keeps the narrow window and
 * the cells outside it read the tables through the vector L1 - 1.6x the kernel's time on such a grid).  Results do not depend on it
 * (bit for bit).  Returns the previous value. */
int rrtmg_lw_hip_set_wide_window(int on);

/* k_layer takes the sixteen bands of a (window of 256 columns, layer) in ONE workgroup - a 100 us chain; a batch with too few such pairs to
 * fill the chip (up to ~2 000 columns of 72 layers) spreads them over two or four workgroups along the staging passes (default on,
 * RRTMG_LW_LAYER_SPLIT=0 to switch off).  Results do not depend on it (bit for bit).  Returns the previous value. */
int rrtmg_lw_hip_set_layer_split(int on);
/* The sweeps decide per wavefront - 64 consecutive columns of a batch - where the clouds end; one deep tower among 64 shallow columns sends
 * all of them through the cloud-zone sweep up to its top.  By default (RRTMG_LW_COLSORT=0 to switch off) the columns of a cloudy batch
 * - rtrn, rtrnmr and the McICA entries, where the key is the grid-mean cloud fraction the sub-columns are drawn from - are therefore
 * TAKEN in another order than they lie: within each window of 256 consecutive columns by their highest cloudy layer,
 * deepest first (k_colsort); the caller's arrays stay as they are and are read / written through that order.  A window is reordered only
 * where that takes at least `min_gain` block-levels out of the cloud zone (sum over its four 64-column blocks of the highest cloudy layer,
 * as the columns lie against sorted; default 24, RRTMG_LW_COLSORT_MIN; < 0 keeps the value): reading the caller's arrays out of order has a
 * price.  on = 1 / off = 0; results do not depend on it (bit for bit).  Returns the previous `on`. */
int rrtmg_lw_hip_set_column_sort(int on, int min_gain);
/* the threshold in force (min_gain above; values beyond 2^24 are taken as 2^24 = never) */
int rrtmg_lw_hip_column_sort_min(void);
/* A block of 64 columns that holds no cloud at all once its window is sorted, and did as the columns lie, is worth more than the levels of
 * its top: where its group of twelve sorted blocks is cloud-free it is swept like a cloud-free call (below).  `percent` of nlay block-levels
 * are added to the window's gain for each such block (0 .. 1000; default 18, i.e. 12 block-levels at 72 layers; 0: the criterion above; RRTMG_LW_COLSORT_CLEAR).  Results do not
 * depend on it (bit for bit).  Returns the previous value; rrtmg_lw_hip_column_sort_clear() the value in force. */
int rrtmg_lw_hip_set_column_sort_clear(int percent);
int rrtmg_lw_hip_column_sort_clear(void);
/* The sweeps of a cloudy batch hand over per group of twelve sorted 64-column blocks at the group's highest cloud.  A group that holds no
 * cloud in any column is swept like a cloud-free call - one clear-sky launch over the whole column, one stream, 8-byte partials - and
 * leaves the three cloudy launches (default on, RRTMG_LW_CLEAR_GROUPS=0 to switch off: such a group then goes through all three with two
 * identical streams).  Results do not depend on it (bit for bit).  Returns the previous value. */
int rrtmg_lw_hip_set_clear_groups(int on);
/* Bytes of device memory the library holds right now, over all its devices: per-batch workspace (it holds what the call shapes seen so far need and only
 * grows: per column of the batch at 72 layers 62 KB for cloud-free calls, 148 KB for rtrnmr, 152 KB for rtrn, 166 KB with idrv = 1; 310 KB at
 * 137 layers with idrv = 1: rrtmg_lw_hip_set_batch trades it against launch count), host-entry staging, McICA masks, the slab buffer
 * (<= 512 MB, or one slab) and the cached chunk states (<= 2 x 180 MB) of the Mersenne-Twister stream. */
long long rrtmg_lw_hip_workspace_bytes(void);
/* Measurement only: 1 = cloud-free GCM calls take the prototype of the "one column per wavefront" mapping (k_n1, profiles/round2_n1_expf.md)
 * instead of the production sweeps.  Off after every rrtmg_lw_hip_init; rrtmg_lw_hip_n1_prototype() reports it. */
int rrtmg_lw_hip_set_n1_prototype(int on);
int rrtmg_lw_hip_n1_prototype(void);
/* Number of g-point chunks the sweep kernel distributes over threads (one partial flux slab each). */
int rrtmg_lw_hip_num_chunks(void);
/* g-points of this build: 140 (librrtmg_lw_hip.so, the reference's shipped model) or 256 (librrtmg_lw_hip_g256.so: every band keeps its 16
 * original g-points - the accuracy mode the reference keeps commented out in modules/parrrtm.f90:40-41,77-110; same symbols; the McICA
 * sub-column arrays and masks then hold 256 sub-columns; select it by linking / loading that library instead). */
int rrtmg_lw_hip_gpoints(void);

/* Per-kernel timing with HIP events recorded on the launch stream (used by bench.py's roofline leg).
 * profile_end synchronises the device and writes "<kernel> <launches> <total_ms>" lines into buf. */
void rrtmg_lw_hip_profile_begin(void);
int rrtmg_lw_hip_profile_end(char *buf, int len);

/* Optional: pin a host array that will be passed to the host-pointer entries again and again (hipHostRegister).  Their H2D / D2H
 * copies then run as asynchronous DMA overlapped with the kernels of the neighbouring column batches. */
int rrtmg_lw_hip_host_register(void *ptr, long long bytes);
int rrtmg_lw_hip_host_unregister(void *ptr);
/* 1 when [ptr, ptr + bytes) lies inside a range registered above - the only arrays the entries copy from where they lie; everything else
 * goes through the library's own pinned staging (an array is NOT pinned because its ends share pages with registered neighbours). */
int rrtmg_lw_hip_host_is_registered(const void *ptr, long long bytes);
/* Optional: declare [ptr, ptr + bytes) STATIC - its contents stay as they are until rrtmg_lw_hip_host_changed(ptr, .).  The host-pointer
 * entries look at every input row of every call for "one value for all columns of the batch" (such rows are filled on the device instead
 * of copied: well-mixed gases handed over as full arrays, zero aerosol and cloud rows); that scan reads ~14 KB per 72-layer column and bounds
 * the entries once the arrays are pinned.  For a static array the answer is kept per (array, column batch) and its rows are not read again.
 * An array that is not declared is scanned on every call (the reference's semantics: inputs may change between calls).
 * rrtmg_lw_hip_host_changed: the contents have changed - the cached scans are dropped; keep = 0 also withdraws the declaration (call it
 * before the array is freed).  Fortran: rrtmg_lw_static / rrtmg_lw_changed (module rrtmg_lw_init). */
int rrtmg_lw_hip_host_static(const void *ptr, long long bytes);
int rrtmg_lw_hip_host_changed(const void *ptr, int keep);
/* Concurrent callers of rrtmg_lw_hip_run_nomcica (an OpenMP host model calling per chunk of columns from several threads, the reference's
 * calling model: serial inside a call, src/rrtmg_lw_rad.nomcica.f90:472): a call of at most RRTMG_LW_COMBINE_MAX (default 8192) columns
 * that finds another call in flight is left in a list; whoever holds the turn solves everything that has gathered with the same
 * (nlay, icld, idrv, inflglw, iceflglw, liqflglw) as ONE device pass and wakes the owners.  Results do not depend on it; a physics error
 * is reported to the call whose columns caused it.  RRTMG_LW_COMBINE=0 restores the plain lock.  This returns the calls that came through
 * the combining entry and the device passes that served them, since the library was loaded. */
void rrtmg_lw_hip_combine_stats(long long *calls, long long *passes);

/* ---- Gas optics and Planck sources -----------------------------------------------------------------------------------------------
 * What the solver forms between its inputs and its sweeps, for hosts with a solver of their own (scattering, multi-stream, "gas optics +
 * sources" interop) and for emulator training data.  No cloud or aerosol arrays are taken and none of the solver's outputs formed.
 *   taug  (ncol, nlay, NG)       taumol's taug(lay, ig) (src/rrtmg_lw_taumol.f90): the GAS optical depth only - no aerosol, no diffusivity
 *                                secant (secdiff), no clamp: a negative interpolated value stays negative.  NG = rrtmg_lw_hip_gpoints()
 *                                (140, or 256 in librrtmg_lw_hip_g256.so); g-points band by band as in the reference.  Band 16 above
 *                                laytrop as the reference forms it: with nspb(16) = 0 (src/rrtmg_lw_init.f90:228) its table indices are 1
 *                                in every layer (absb rows 1 and 2 with the layer's weights); the solver itself indexes that table by (jp, jt).
 *   fracs (ncol, nlay, NG)       taumol's Planck fraction per g-point.  (The solver's sweeps carry the mixture weight of the binary-key bands
 *                                in 28 bits; these are formed with the full weight, as the reference forms them.)
 *   planklay (ncol, nlay, 16)    setcoef's planklay;  planklev (ncol, nlay+1, 16): setcoef's planklev(0:nlay), level 0 = the surface
 *   plankbnd (ncol, 16)          setcoef's plankbnd, which includes semiss (emis);  dplankbnd_dt (ncol, 16): its d/dT
 *                                (src/rrtmg_lw_setcoef.f90:173-269).  Band 16 as in a broadband call (istart = 1), like the spectral outputs.
 * Layout: column fastest, the g-point or band index last: element (i, k, g) at i + ncol*(k + nlay*g) (0-based), like tauaer and the
 * spectral outputs.  Layer 1 is the surface layer.  The solver's own optical depth of a cell is secdiff(band) * (taug + taua(band)).
 * taug and fracs are required.  Each Planck output may be NULL: it is then neither formed nor stored.  dplankbnd_dt is required with
 * idrv = 1; with idrv = 0 it may be NULL and is left untouched.  Inputs as for rrtmg_lw_hip_run_nomcica (inatm's hydrostatic amounts);
 * errors: RRTMG_LW_HIP_EARG for null required arrays and bad dimensions (the limits of the other entries).
 * The host entry splits the columns over the devices of rrtmg_lw_hip_init_devices like rrtmg_lw_hip_run_nomcica.  The device entry takes
 * device pointers laid out as above, enqueues on `stream`, runs on the state of the arrays' device and does not synchronise:
 * rrtmg_lw_hip_check(stream) reports errors, as for the other device entries.  These entries take the entry lock like any other call
 * (no combining, no graph replay). */
int rrtmg_lw_hip_gas_optics(int ncol, int nlay, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis,
    double *taug, double *fracs, double *planklay, double *planklev, double *plankbnd, double *dplankbnd_dt);
int rrtmg_lw_hip_gas_optics_device(int ncol, int nlay, int idrv,
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr,
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,
    const double *ccl4vmr, const double *emis,
    double *taug, double *fracs, double *planklay, double *planklev, double *plankbnd, double *dplankbnd_dt, void *stream);
/* The same for prepared columns: the arguments of rrtmg_lw_hip_run_columns up to pwvcm (src/rrtmg_lw.1col.f90:497-580, semiss in place of
 * emis); at most one batch of columns per call, like rrtmg_lw_hip_run_columns. */
int rrtmg_lw_hip_gas_optics_columns(int ncol, int nlayers, int idrv,
    const double *pavel, const double *tavel, const double *pz, const double *tz, const double *tbound,
    const double *semiss, const double *coldry, const double *wkl, const double *wbrodl, const double *wx,
    const double *pwvcm,
    double *taug, double *fracs, double *planklay, double *planklev, double *plankbnd, double *dplankbnd_dt);

/* ---- Device arrays in the host model's own form --------------------------------------------------------------------------------------
 * The device-pointer entries above take the reference's array form only: float64, columns fastest, layer 1 at the surface.  A
 * device-resident caller that holds float32 values, C-order (column, level) storage or a top-down vertical index describes its arrays
 * once and hands them over as they lie; the library converts them on the device, in one kernel per column batch in front of the solver
 * and one behind it, and returns the results in the same form.
 *   real_bytes      8: float64.  4: float32 - EVERY floating-point array of the call, inputs and outputs.  Inputs are widened (exact),
 *                   outputs are the float64 results rounded to nearest, (float)x.
 *   layer_fastest   0: each array as the plain entry declares it (taucld (16,ncol,nlay) and tauaer (ncol,nlay,16) included).
 *                   1: every array in C order with the column index FIRST (slowest) and everything else behind it:
 *                        play, tlay, the gases, cldfr, cicewp, cliqwp, reice, reliq, alpha, hr, hrc      (ncol, nlay)
 *                        plev, tlev, uflx, dflx, uflxc, dflxc, duflx_dt, duflxc_dt                       (ncol, nlay+1)
 *                        emis, plankbnd, dplankbnd_dt                                                    (ncol, 16)
 *                        taucld, tauaer, planklay                                                        (ncol, nlay, 16)
 *                        planklev                                                                        (ncol, nlay+1, 16)
 *                        taug, fracs                                                                     (ncol, nlay, NG), NG = rrtmg_lw_hip_gpoints()
 *                        tsfc                                                                            (ncol)
 *   top_first       0: index 0 of the vertical axis at the surface.  1: at the top of the atmosphere - layer k of the reference lies at
 *                   nlay-1-k, level k at nlay-k; inputs and outputs, in both layouts.
 * Each entry takes the argument list of the entry it is named after behind `form`, its arrays as const void * / void *: icld and irng
 * in / out, the flags, the NULL rules of optional outputs (a NULL output is neither formed nor touched), `stream`, no synchronisation,
 * errors through rrtmg_lw_hip_check(stream) and rrtmg_lw_hip_last_error() with the same texts.  The device is chosen from `play`.
 * Results: what the plain entry gives on the same values brought into the reference form - float32 inputs widened, float32 outputs
 * rounded - bit for bit.  The form {8, 0, 0} forwards to the plain entry.  RRTMG_LW_HIP_EARG: a null `form`, real_bytes other than 4 or 8,
 * a flag other than 0 or 1, a null required array.  The output arrays must not overlap the inputs.
 * The batch's arrays are staged in device memory the library owns (counted in rrtmg_lw_hip_workspace_bytes; per column of a batch the
 * float64 reference form of the call's arrays, taucld as one band sum per cell where inflglw >= 1; the fused McICA entry also holds play,
 * cldfr and alpha of the whole call for its generator).  The batches run one after the other on `stream`; such calls are not replayed as
 * graphs.  Out of scope: the explicit-sub-column McICA entries, the spectral outputs and the queue; HOST arrays of a host built with
 * 4-byte reals have entries of their own (the "_r4" section below; reference layout only - a Fortran host is column-fastest by nature). */
typedef struct {
    int real_bytes;
    int layer_fastest;
    int top_first;
} rrtmg_lw_hip_array_form;

int rrtmg_lw_hip_run_nomcica_device_as(const rrtmg_lw_hip_array_form *form,
    int ncol, int nlay, int *icld, int idrv,
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,
    const void *ccl4vmr, const void *emis, int inflglw, int iceflglw, int liqflglw,
    const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp,
    const void *reice, const void *reliq, const void *tauaer,
    void *uflx, void *dflx, void *hr, void *uflxc, void *dflxc, void *hrc,
    void *duflx_dt, void *duflxc_dt, void *stream);
int rrtmg_lw_hip_run_mcica_subcol_device_as(const rrtmg_lw_hip_array_form *form,
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,
    const void *ccl4vmr, const void *emis, int inflglw, int iceflglw, int liqflglw,
    const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp,
    const void *reice, const void *reliq, const void *alpha, const void *tauaer,
    void *uflx, void *dflx, void *hr, void *uflxc, void *dflxc, void *hrc,
    void *duflx_dt, void *duflxc_dt, void *stream);
int rrtmg_lw_hip_gas_optics_device_as(const rrtmg_lw_hip_array_form *form, int ncol, int nlay, int idrv,
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,
    const void *ccl4vmr, const void *emis,
    void *taug, void *fracs, void *planklay, void *planklev, void *plankbnd, void *dplankbnd_dt, void *stream);

/* ---- Surface-temperature adjustment of idrv = 1 results -----------------------------------------------------------------------------
 * With idrv = 1 the rrtmg_lw entries return duflx_dt and duflxc_dt, "to approximate adjustments to the upward flux profile caused only by
 * a change in surface temperature between full radiation calls" (src/rrtmg_lw_rad.nomcica.f90:161-171).  These entries apply them, as
 * the reference's column driver does (src/rrtmg_lw.1col.f90:582-610): a host that calls radiation every N-th step keeps the fluxes of
 * that call and, on each step between, hands them over with its current surface temperature.  In float64, per column i and level k:
 *     uflx_adj(k) = uflx(k) + duflx_dt(k) * dtsfc(i)        (the product rounded, then the sum: no fused multiply-add)
 *     net(k)      = uflx_adj(k) - dflx(k)
 *     hr_adj(l)   = heatfac * (net(l) - net(l+1)) / (plev(l) - plev(l+1)),   l = 0 .. nlay-1
 * and the same for the clear-sky set (uflxc, dflxc, duflxc_dt -> uflxc_adj, hrc_adj).  dtsfc (ncol) is the current surface temperature
 * minus the tsfc of the radiation call that produced the fluxes; heatfac is that of the initialisation (cpdair).  The inputs are always
 * the STORED, unadjusted fluxes of that call: an adjustment is not cumulative.  Downward fluxes do not change and are not output.  With
 * dtsfc = 0 the outputs are the solver's own uflx and hr, bit for bit (its heating rate is formed by the same expression).
 * Arrays: plev and the flux arrays (ncol,nlay+1), hr_adj and hrc_adj (ncol,nlay), dtsfc (ncol); columns fastest, level 0 at the surface.
 * The five clear-sky arrays are all NULL - then none is read or written - or all set.  No output may overlap an input or another output
 * (the address ranges are compared).  RRTMG_LW_HIP_EARG: a null required array, some but not all of the clear-sky arrays, an overlap,
 * dimensions outside the limits of the other entries; nothing is written then.
 *   rrtmg_lw_hip_adjust_tsfc            HOST pointers.  Takes the entry lock, splits the columns over the devices of
 *                                       rrtmg_lw_hip_init_devices and moves them through the pipeline of the other host entries
 *                                       (registered arrays are copied from where they lie).  The results do not depend on the batch
 *                                       size or on the number of devices (bit for bit).
 *   rrtmg_lw_hip_adjust_tsfc_device     DEVICE pointers.  One kernel launch on `stream`, on the state of the device `plev` lives on; no
 *                                       workspace, no synchronisation; errors through rrtmg_lw_hip_check(stream) like the other device
 *                                       entries.
 *   rrtmg_lw_hip_adjust_tsfc_device_as  the same for arrays in the caller's form (rrtmg_lw_hip_array_form above, all three fields; with
 *                                       real_bytes = 4 every array is float32, dtsfc included: inputs widened, the arithmetic above in
 *                                       float64, outputs rounded, (float)x).  The kernel reads and writes the caller's arrays where
 *                                       they lie - nothing is staged or converted.  {8, 0, 0} forwards to the plain device entry; form
 *                                       errors as in the other *_as entries. */
int rrtmg_lw_hip_adjust_tsfc(int ncol, int nlay, const double *plev, const double *dtsfc,
    const double *uflx, const double *dflx, const double *duflx_dt,
    const double *uflxc, const double *dflxc, const double *duflxc_dt,
    double *uflx_adj, double *hr_adj, double *uflxc_adj, double *hrc_adj);
int rrtmg_lw_hip_adjust_tsfc_device(int ncol, int nlay, const double *plev, const double *dtsfc,
    const double *uflx, const double *dflx, const double *duflx_dt,
    const double *uflxc, const double *dflxc, const double *duflxc_dt,
    double *uflx_adj, double *hr_adj, double *uflxc_adj, double *hrc_adj, void *stream);
int rrtmg_lw_hip_adjust_tsfc_device_as(const rrtmg_lw_hip_array_form *form, int ncol, int nlay, const void *plev, const void *dtsfc,
    const void *uflx, const void *dflx, const void *duflx_dt,
    const void *uflxc, const void *dflxc, const void *duflxc_dt,
    void *uflx_adj, void *hr_adj, void *uflxc_adj, void *hrc_adj, void *stream);

/* ---- Device arrays with a column stride ("_view") ------------------------------------------------------------------------------------
 * A GPU-resident host model dimensions its fields (pcols, pver) and calls radiation for ncol <= pcols columns of them, or for a range
 * of columns out of a wider field.  These four entries take such arrays where they lie: the array form of the *_as entries above
 * (real_bytes, layer_fastest, top_first: the same meaning) plus
 *   ld              the column extent of EVERY column-fastest array of the call, inputs and outputs alike, in elements: element (i, k)
 *                   of a (ncol, nlay) array lies at i + ld*k.  emis and plankbnd are (ld, 16); taucld (16, ld, nlay): element (b, i, k) at
 *                   b + 16*(i + ld*k); tauaer and planklay (ld, nlay, 16): element (i, k, b) at i + ld*(k + nlay*b); the spectral outputs
 *                   and planklev (ld, nlay+1, 16); taug and fracs (ld, nlay, NG); tsfc and dtsfc (ncol).  The vertical extent stays nlay /
 *                   nlay+1 as passed (no vertical stride).  ld = 0 means ncol.  ld < ncol is RRTMG_LW_HIP_EARG.  The largest ld is
 *                   2^30 = 1 073 741 824; a larger one is RRTMG_LW_HIP_EARG (every product with ld is formed in 64 bits; the bound keeps
 *                   ld plus a batch's column offset inside 32 bits).  With layer_fastest = 1 the column is the slowest index and a
 *                   column range is a pointer offset and nothing else: ld must be 0 or ncol, anything else is RRTMG_LW_HIP_EARG.
 * Pointers: every pointer addresses the element of the FIRST COLUMN OF THE CALL - for columns [c0, c0 + ncol) of a wider field the caller
 * passes p + c0 (taucld: p + 16*c0; with layer_fastest = 1, p + c0 * the column's values).  The device is chosen from `play` (plev in
 * the adjustment entry).  Each entry takes the argument list of the *_as entry it is named after behind `view`; the two solver entries
 * take four more outputs in front of `stream`:
 *   uflxs, dflxs, uflxcs, dflxcs    the spectral outputs of the *_spectral entries, (ld, nlay+1, 16) ((ncol, nlay+1, 16) in C order with
 *                   layer_fastest = 1), in the view's element type, vertical order and layout.  All four NULL: the plain call.  Otherwise
 *                   the rules of the *_spectral entries: uflxs and dflxs both set, uflxcs and dflxcs both NULL or both set.
 * Results: what the existing entry of the same form returns on contiguous copies of the call's ncol columns (*_device, *_spectral_device,
 * *_device_as), bit for bit.  Elements outside the call's columns - the padding of each row, the other columns of a wider field - are
 * never written, and their contents never influence a result (they may hold NaN).
 * The form {8, 0, 0} runs IN PLACE: the solver's kernels read and write the caller's arrays with ld as their row stride, nothing is
 * staged, the call keeps the pipelining and the graph replay of the plain device entry (ld is part of a graph's key), and
 * rrtmg_lw_hip_workspace_bytes() is what the plain entry of the same shape leaves.  One exception: the fused McICA entry with irng = 1
 * and ld != ncol copies play, cldfr and alpha of the call into ncol-wide arrays of its own first (3 x ncol x nlay x 8 B), as the *_as
 * entry does - the Mersenne-Twister stream is consumed over the ncol columns of the call, in call order.  {8, 0, 0} with ld = 0 or ncol
 * is the plain (or spectral) device entry.  The adjustment entry reads and writes in place in every form; it moves 16 bytes per access
 * where every row of every array starts on a 16-byte boundary and one element otherwise (an odd first column or an odd ld).
 * A converting form (float32, top first, layer fastest) goes through the staging of the *_as entries; the spectral outputs, when asked
 * for, are staged like the others: 4 x (nlay+1) x 16 x 8 B more per column of a batch (2 x without the clear-sky pair), allocated only
 * then.  Errors (RRTMG_LW_HIP_EARG, refused before anything is launched): a null view, the form errors of the *_as entries, the ld
 * rules above, a half-given spectral pair, and everything the entry named after refuses.
 * Out of scope: the explicit-sub-column McICA entries, the queue, host pointers, a vertical stride. */
typedef struct {
    int real_bytes;
    int layer_fastest;
    int top_first;
    int ld;
} rrtmg_lw_hip_array_view;

int rrtmg_lw_hip_run_nomcica_device_view(const rrtmg_lw_hip_array_view *view,
    int ncol, int nlay, int *icld, int idrv,
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,
    const void *ccl4vmr, const void *emis, int inflglw, int iceflglw, int liqflglw,
    const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp,
    const void *reice, const void *reliq, const void *tauaer,
    void *uflx, void *dflx, void *hr, void *uflxc, void *dflxc, void *hrc,
    void *duflx_dt, void *duflxc_dt, void *uflxs, void *dflxs, void *uflxcs, void *dflxcs, void *stream);
int rrtmg_lw_hip_run_mcica_subcol_device_view(const rrtmg_lw_hip_array_view *view,
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,
    const void *ccl4vmr, const void *emis, int inflglw, int iceflglw, int liqflglw,
    const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp,
    const void *reice, const void *reliq, const void *alpha, const void *tauaer,
    void *uflx, void *dflx, void *hr, void *uflxc, void *dflxc, void *hrc,
    void *duflx_dt, void *duflxc_dt, void *uflxs, void *dflxs, void *uflxcs, void *dflxcs, void *stream);
int rrtmg_lw_hip_gas_optics_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int idrv,
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,
    const void *ccl4vmr, const void *emis,
    void *taug, void *fracs, void *planklay, void *planklev, void *plankbnd, void *dplankbnd_dt, void *stream);
int rrtmg_lw_hip_adjust_tsfc_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, const void *plev, const void *dtsfc,
    const void *uflx, const void *dflx, const void *duflx_dt,
    const void *uflxc, const void *dflxc, const void *duflxc_dt,
    void *uflx_adj, void *hr_adj, void *uflxc_adj, void *hrc_adj, void *stream);
/* The mean over nsamp sub-column samples ("The mean over several sub-column samples", above) of DEVICE arrays in the view's form, and
 * optionally the sample variances uflx_var, dflx_var, hr_var in the same form (hr_var flips with top_first like hr; a float32 output is
 * the float64 result rounded once, after the last sample).  All three NULL: the mean alone.  {8, 0, 0, 0}: the plain
 * rrtmg_lw_hip_run_mcica_samples_device, plus variance.  {8, 0, 0, ld} runs in place, sample by sample on the caller's arrays; a
 * converting form stages a batch's inputs (alpha too) once, runs the samples on the staged arrays and converts the outputs once.  The
 * results are those of rrtmg_lw_hip_run_mcica_samples_device on float64 reference-form copies of the call's columns, put into the form.
 * No spectral arguments.  Errors: those of that entry and of the view, and the two variance cases.  Enqueues on `stream`, does not
 * synchronise; a physics error surfaces through rrtmg_lw_hip_check(stream). */
int rrtmg_lw_hip_run_mcica_samples_device_view(const rrtmg_lw_hip_array_view *view,
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int nsamp, int seedstep, int *irng,
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,
    const void *ccl4vmr, const void *emis, int inflglw, int iceflglw, int liqflglw,
    const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp,
    const void *reice, const void *reliq, const void *alpha, const void *tauaer,
    void *uflx, void *dflx, void *hr, void *uflxc, void *dflxc, void *hrc,
    void *duflx_dt, void *duflxc_dt, void *uflx_var, void *dflx_var, void *hr_var, void *stream);
/* rrtmg_lw_hip_get_alpha on DEVICE arrays in the view's form: dz, cldfrac and alpha are layer arrays ((ld, nlay), or (ncol, nlay) in C
 * order with layer_fastest = 1), lat is per column.  The value of reference layer k is stored where the form keeps layer k.  Float64
 * arithmetic, the host entry's bits in the form {8, 0, 0}; a float32 alpha is that value rounded.  Enqueues on `stream`, does not
 * synchronise.  icld other than 4 or 5: returns 0 and leaves alpha alone, like the host entry.  lat may be NULL unless idcor = 1. */
int rrtmg_lw_hip_get_alpha_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int icld, int idcor, double decorr_con,
    const void *dz, const void *lat, int juldat, const void *cldfrac, void *alpha, void *stream);

/* ---- Cloud cover as the McICA sub-columns realise it -----------------------------------------------------------------------------------
 * The fused entries (rrtmg_lw_hip_run_mcica_subcol*, rrtmg_lw_hip_run_mcica_samples*) draw their sub-columns on the device and keep them
 * as a packed mask only.  These three entries run the same generator stage - deterministic in (icld, permuteseed, irng, play, cldfr,
 * alpha) - and count that mask, so they report exactly the clouds a fused call with the same arguments saw: a model that diagnoses total
 * or low / mid / high cover inside radiation gets numbers that agree with the fluxes, a satellite simulator gets the sub-columns
 * themselves, and neither materialises the (NG, ncol, nlay) arrays of rrtmg_lw_hip_mcica_subcol (about 80 KB per 72-layer column for
 * cldfmcl alone, against 20 bytes per column and layer of mask).  No solver kernel runs.
 * With NG = rrtmg_lw_hip_gpoints(), sample s drawn with the seed permuteseed + s * seedstep as the averaging entries define it, and
 * c(i, k, g, s) in {0, 1} the generator's cldfmcl of column i, layer k (layer 1 at the surface), sub-column g:
 *     cldtot  (ncol)          the pairs (g, s) with c = 1 in at least one layer, / (NG * nsamp)
 *     cldcum  (ncol,nlay)     for layer k the pairs with c = 1 in some layer k' >= k, / (NG * nsamp): the cover seen from the top of the
 *                             atmosphere down to and including layer k.  cldcum(:,1) = cldtot; it does not increase with k.  High /
 *                             mid / low cover as seen from above are differences of its rows: with k_hi and k_mid the lowest layers
 *                             of the high and the middle deck, high = cldcum(:,k_hi), mid = cldcum(:,k_mid) - cldcum(:,k_hi) (what
 *                             the middle deck adds below the high one), low = cldtot - cldcum(:,k_mid); the three add up to cldtot
 *     cldlay  (ncol,nlay)     the pairs with c(i, k, g, s) = 1, / (NG * nsamp): the realised layer fraction, to be held against cldfr
 *     submask (ncol,nlay,MW)  unsigned 32-bit, MW = (NG + 31) / 32: bit (g mod 32) of word g / 32 is c(i, k, g, 0); the bits at and
 *                             above NG are zero.  With nsamp = 1 only.
 * Each output may be NULL - it is then neither formed nor touched -, at least one must be given.  Every count is an exact integer and
 * every value ONE IEEE float64 division (double)count / (double)(NG * nsamp) - not a multiplication by a reciprocal -, for a float32
 * array rounded once more with (float): any implementation of the definitions agrees bit for bit.
 * icld, irng (in/out: any non-zero value becomes 1), the limits of nlay and alpha (NULL unless icld is 4 or 5) are those of
 * rrtmg_lw_hip_mcica_subcol_device; icld = 0 writes exact zeros to every given output (radiation saw no cloud) and reads no input.
 * nsamp and seedstep follow rrtmg_lw_hip_run_mcica_samples, with its error texts: nsamp in 1 .. RRTMG_LW_HIP_MAX_SAMPLES, seedstep >= 1,
 * the last seed an int, *irng = 0 with nsamp > 1.  RRTMG_LW_HIP_EARG as well, with a text that names the argument: all four outputs
 * NULL, submask together with nsamp > 1, play or cldfr NULL (icld != 0), alpha NULL with icld 4 / 5.  Every such case is found before
 * any output is written.
 * Device entries: DEVICE pointers, the device is that of play (rrtmg_lw_hip_init_devices; with icld = 0 and play NULL that of the
 * first output given); they enqueue on `stream` and do not
 * synchronise, a physics error (kissvec: pressures that do not decrease upward) surfaces through rrtmg_lw_hip_check(stream).  The masks
 * of all columns of the call are drawn at once into the buffer the fused entries use (20 B per column and layer, 32 in the g256
 * library; counted by rrtmg_lw_hip_workspace_bytes), the jump tables are the fused entries' - a seed they have seen rebuilds nothing,
 * and the other way round.  Per sample the generator and one counting kernel run; the counts add up in the output arrays (sample 0
 * stores, the others add, the last one adds and divides: counts are at most 256 x 64, exact in float32 too), which are never read
 * before they are written.  The entry lock, no graph replay, no combining with other calls, no column batches (rrtmg_lw_hip_set_batch
 * does not apply).
 * rrtmg_lw_hip_mcica_cloud_cover_device_view: inputs and floating-point outputs in the view's form ("Device arrays with a column
 * stride", above) exactly as rrtmg_lw_hip_get_alpha_device_view takes (ncol,nlay) arrays; cldtot is per column, like tsfc.  submask is
 * always unsigned 32-bit: (ld, nlay, MW) column-fastest - word w of layer k of column i at i + ld * (k + nlay * w) -, or, with
 * layer_fastest = 1, (ncol, nlay, MW) in C order - at (i * nlay + k) * MW + w.  With top_first = 1 the vertical index k is flipped in
 * both layouts, as in every other array; "this layer or any above it" is physical and does not flip.  {8, 0, 0, ld} runs on the caller's
 * arrays in place (irng = 1 with ld > ncol copies play, cldfr and alpha call-wide first, as the fused view entry does); a converting
 * form stages those three call-wide in float64 and the counting kernel writes the outputs in the form directly.  Nothing outside the
 * call's ncol columns is read into a result or written.
 * rrtmg_lw_hip_mcica_cloud_cover: HOST pointers, reference layout.  The first device, no fan-out over several devices.  It allocates
 * one device buffer for the call - play, cldfr, alpha (icld 4 / 5) and the outputs that are given: 8 B per column and layer each, 8 B
 * per column for cldtot, 4 MW B per column and layer for submask - beside the mask buffer, releases it when it returns, and copies
 * the outputs back.  Synchronises. */
int rrtmg_lw_hip_mcica_cloud_cover(int ncol, int nlay, int icld, int permuteseed, int nsamp, int seedstep, int *irng,
    const double *play, const double *cldfr, const double *alpha,
    double *cldtot, double *cldcum, double *cldlay, unsigned *submask);
int rrtmg_lw_hip_mcica_cloud_cover_device(int ncol, int nlay, int icld, int permuteseed, int nsamp, int seedstep, int *irng,
    const double *play, const double *cldfr, const double *alpha,
    double *cldtot, double *cldcum, double *cldlay, unsigned *submask, void *stream);
int rrtmg_lw_hip_mcica_cloud_cover_device_view(const rrtmg_lw_hip_array_view *view,
    int ncol, int nlay, int icld, int permuteseed, int nsamp, int seedstep, int *irng,
    const void *play, const void *cldfr, const void *alpha,
    void *cldtot, void *cldcum, void *cldlay, unsigned *submask, void *stream);

/* ---- Cloud optics: band optical depths, ncbands, secdiff ---------------------------------------------------------------------------------
 * The gas-optics entries give the gas optical depth per g-point and the cloud-cover entries the McICA sub-columns; these three give the
 * remaining pieces of the solver's optical depth: the cloud optical depth per spectral band that cldprop (imca = 0) or cldprmc
 * (imca = 1) forms from water paths and particle sizes, BEFORE the diffusivity secant; cldprop's band count; and the secants.  No solver
 * kernel runs, and the solver's own cloud kernels are not the ones used here.
 * Every value is float64 arithmetic in which each operation rounds on its own (no fused multiply-add) and every division is an IEEE
 * division, so that any implementation of the definitions below agrees to the bit.  Inputs as in rrtmg_lw_hip_run_nomcica: cldfr, cicewp,
 * cliqwp, reice, reliq, h2ovmr (ncol,nlay), taucld (16,ncol,nlay), plev (ncol,nlay+1), the flags inflglw, iceflglw, liqflglw.
 *   taucloud (ncol,nlay,16)   laid out like tauaer.
 *     imca = 0 (src/rrtmg_lw_cldprop.f90:50-295): for spectral band B of layer k the reference's taucloud(k, ib) with ib = ipat(B, .) for
 *       the column's FINAL ncbands (the map of src/rrtmg_lw_rtrn.f90:343-349): the cloud optical depth the sweeps use for the g-points of
 *       band B.  Zero except in layers that enter cldprop: cldfr >= 1e-20 and (cicewp + cliqwp >= 1e-20 or the sum of taucld over the
 *       bands, added in band order, >= 1e-20).  In an entering layer only the cloud bands ib <= the band count cldprop had reached AT THAT
 *       LAYER (walking up from the surface) are assigned: a layer worked on while ncbands was 1 stays zero in cloud bands 2..16 even if a
 *       later layer raises the count.  inflglw = 0: taucld(ib); 1: abscld1 * (cicewp + cliqwp); 2: cicewp * abscoice(ib) + cliqwp *
 *       abscoliq(ib) with cldprop's table positions, iceind / liqind maps and 1 -> 2 promotion, every interpolation
 *       tb[i-1] + fint * (tb[i] - tb[i-1]).  The library's one stated deviation holds here too: in an ice-only layer with iceflglw = 1 of
 *       a 16-band column, cloud bands 6-16 use the fifth Ebert-Curry band.  Layers with 1e-20 <= cldfr < 1e-6 get their cldprop value
 *       although the sweeps treat them as cloud-free and never read it.
 *     imca = 1 (src/rrtmg_lw_cldprmc.f90:49-279 on the sub-columns the generator expands from grid-mean inputs): what cldprmc leaves in
 *       taucmc(ig, k) for a CLOUDY sub-column ig of band B; it does not depend on the mask.  Formed in layers with cldfr >= 1e-20 (below
 *       that the generator draws no cloudy sub-column; the value is zero).  A cell enters when cicewp + cliqwp >= 1e-20 or taucld(B) >=
 *       1e-20; one that does not keeps taucld(B).  An entering cell: inflglw = 0: taucld(B); 2: cicewp * abscoice(B) + cliqwp *
 *       abscoliq(B), iceflglw = 1 through the five-band map per band; 1: the reference's stop (below).
 *   ncbands (ncol)            int32 whatever the form: imca = 0: cldprop's band count at the end of the column, 1, 5 or 16; imca = 1: 16.
 *   secdiff (ncol,16)         laid out like emis: the diffusivity secant of each band (rtrn :280-288): 1.66 in bands 1, 4 and 10-16,
 *                             a0 + a1 * exp(a2 * pwvcm) clamped to [1.5, 1.8] elsewhere, pwvcm the precipitable water of inatm
 *                             (src/rrtmg_lw_rad.nomcica.f90:795-863) from plev and h2ovmr.  The same for both imca values.
 * The solver's cloud term of band B is secdiff(icb) * taucloud(B) with icb = ipat(B, .) of the column's ncbands in the deterministic
 * solver - the reference indexes secdiff by the CLOUD band there (rtrn :323): band 1 for ncbands = 1, bands 1, 2, 3, 3, 3, 4, 4, 4, 5 ...
 * for 5, B for 16 - and secdiff(B) * taucloud(B) for McICA, in the cells the mask marks.
 * Each output may be NULL - it is then neither formed nor touched -, at least one must be given.  The six cloud arrays are required
 * when taucloud or ncbands is given, plev and h2ovmr when secdiff is; arrays a call does not need may be NULL and are not read.
 * Particle sizes: where a size is read - inflglw = 2, the phase's water path non-zero, liquid with liqflglw = 1 - the bounds and texts
 * are the solver's ("Cloud particle sizes"): RRTMG_LW_HIP_EPHYSICS from the host entry's return value, from
 * rrtmg_lw_hip_check(stream) for the device entries.  With imca = 1 a size is checked in EVERY layer with cldfr >= 1e-20 that enters,
 * whether or not a particular seed would draw a cloudy sub-column there (the fused solver entries check only where one is drawn);
 * inflglw = 1 with imca = 1 is the reference's stop "INFLAG = 1 OPTION NOT AVAILABLE WITH MCICA" wherever a cell enters.  The outputs
 * of a failed call are not valid; the next call starts clean.
 * RRTMG_LW_HIP_EARG, with a text that names the argument and before anything is written: imca other than 0 or 1, the dimension limits
 * of the other entries, the view rules, a missing required array, all outputs NULL, an output that shares a byte with a needed input
 * or with another output.
 * Device entries: DEVICE pointers; the device is that of cldfr (of plev when only secdiff is asked for); they enqueue on `stream` and do
 * not synchronise.  The entry lock, no graph replay, no combining.  Two kernels: one thread per column (the band-count walk, pwvcm and
 * secdiff), one thread per (column, layer) (the sixteen band values); (nlay + 1) bytes per column of workspace in the *_as staging buffer.
 * rrtmg_lw_hip_cloud_optics_device_view: the arrays in the view's form ("Device arrays with a column stride", above), all four fields
 * with their meaning there: taucld as in the solver entries, taucloud like tauaer, secdiff like emis, ncbands indexed per column.  Every
 * form is read and written IN PLACE - {8, 0, 0, ld} and the converting ones alike, nothing is staged; a float32 input is widened
 * exactly, a float32 output is the float64 value rounded once.  Nothing outside the call's ncol columns is read into a result or written.
 * rrtmg_lw_hip_cloud_optics: HOST pointers, reference layout, the first device; staged in column batches (rrtmg_lw_hip_set_batch, at
 * most 16 384) through the host-entry staging buffer; the results do not depend on the batch size.  Synchronises. */
int rrtmg_lw_hip_cloud_optics(int ncol, int nlay, int imca, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *plev, const double *h2ovmr,
    double *taucloud, int *ncbands, double *secdiff);
int rrtmg_lw_hip_cloud_optics_device(int ncol, int nlay, int imca, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp,
    const double *reice, const double *reliq, const double *plev, const double *h2ovmr,
    double *taucloud, int *ncbands, double *secdiff, void *stream);
int rrtmg_lw_hip_cloud_optics_device_view(const rrtmg_lw_hip_array_view *view,
    int ncol, int nlay, int imca, int inflglw, int iceflglw, int liqflglw,
    const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp,
    const void *reice, const void *reliq, const void *plev, const void *h2ovmr,
    void *taucloud, int *ncbands, void *secdiff, void *stream);

/* ---- The solver on the caller's optical depths and sources -------------------------------------------------------------------------------
 * The gas-optics, cloud-optics and cloud-cover entries hand out every piece the solver consumes; these two turn such arrays - the
 * library's own, or a host's changed ones (an emulator in place of taumol, another cloud parametrisation, aerosol terms, perturbed
 * optical depths) - back into fluxes and heating rates: the level loops of rtrn (src/rrtmg_lw_rtrn.f90:361-604) and rtrnmc
 * (src/rrtmg_lw_rtrnmc.f90) in float64, each operation rounding on its own, on the float64 tables exp_tbl, tfn_tbl, tau_tbl of
 * src/rrtmg_lw_init.f90:125-142.  Two kernels of their own; the production sweeps and their cell codes are not used.
 * All arrays float64, column-fastest, layer 1 at the surface, laid out as the optics entries write them (NG = rrtmg_lw_hip_gpoints(),
 * MW = (NG + 31) / 32, band of g: ngb):
 *   plev (ncol,nlay+1); emis, plankbnd, dplankbnd_dt (ncol,16); tau, fracs (ncol,nlay,NG); planklay, odcld (ncol,nlay,16);
 *   planklev (ncol,nlay+1,16), level 0 the surface; cldfr (ncol,nlay); submask (ncol,nlay,MW) unsigned 32-bit as
 *   rrtmg_lw_hip_mcica_cloud_cover writes it; the outputs as in rrtmg_lw_hip_run_nomcica.
 *   tau    the clear-sky optical depth along the diffusivity path, secdiff(band of g) * (taug + tauaer(band of g)): the caller forms it.
 *          A negative value is taken as 0 (rtrn :372).
 *   odcld  the cloud optical depth along the same path per spectral band B: from the cloud-optics outputs secdiff(icb) * taucloud(B) for
 *          cloud = 1 and secdiff(B) * taucloud(B) for cloud = 2 ("Cloud optics", above).
 * cloud = 0: cldfr, odcld and submask are not read; the total-sky outputs equal the clear-sky ones.
 * cloud = 1: rtrn, random overlap: layer k is cloudy when cldfr(k) >= 1e-6, with cf = cldfr(k), odc = odcld(k, B) in every g-point of B.
 * cloud = 2: rtrnmc: layer k is cloudy when any of the NG bits of submask(k, .) is set (bits at and above NG are ignored); in cell (k, g)
 *            cf = 1, odc = odcld(k, B) where bit g is set, cf = 0, odc = 0 where it is not.
 * efc = (1 - exp(-odc)) * cf.  Per g-point of band B, with od = max(tau, 0), f = fracs, blay = planklay(k, B), dup = planklev(k, B) - blay
 * (the layer's upper interface), ddn = planklev(k-1, B) - blay, idx(x) = int(1e4 * (x / (bpade + x)) + 0.5), bpade = 1 / 0.278, the
 * division an IEEE division, rec_6 = 0.166667:
 *   a clear layer:  od <= 0.06: atrans = od - 0.5 * od * od, t = rec_6 * od;  else  i = idx(od), atrans = 1 - exp_tbl(i), t = tfn_tbl(i);
 *                   bbd = f * (blay + ddn * t), bbu = f * (blay + dup * t);
 *                   down  rad = rad + (bbd - rad) * atrans;   up  rad = rad + (bbu - rad) * atrans,  drad = drad * (1 - atrans)
 *   a cloudy layer: odtot = od + odc.  odtot < 0.06: atrans, t as above, atot = odtot - 0.5 * odtot * odtot, tt = rec_6 * odtot;
 *                   else od <= 0.06: atrans, t as above, j = idx(odtot), atot = 1 - exp_tbl(j), tt = tfn_tbl(j);
 *                   else i = idx(od), od = tau_tbl(i), atrans = 1 - exp_tbl(i), t = tfn_tbl(i), odtot = od + odc, j, atot, tt as before;
 *                   bbd, bbu as above, bbdtot = f * (blay + ddn * tt), bbutot = f * (blay + dup * tt), gassrc = bbd * atrans going down
 *                   (atrans * f * (blay + t * ddn) in the third case), bbu * atrans going up;
 *                   rad = rad - rad * (atrans + efc * (1 - atrans)) + gassrc + cf * (bb.tot * atot - gassrc);
 *                   up  drad = drad * cf * (1 - atot) + drad * (1 - cf) * (1 - atrans)
 *   The downward radiance starts at 0 above the top layer; at the surface rad = f(1) * plankbnd(B) + (1 - emis(B)) * rad_down and, with
 *   idrv = 1, drad = f(1) * dplankbnd_dt(B).  The clear-sky stream is the total one down to the first cloudy layer met from the top
 *   (iclddn) - in a column without cloud everywhere -; from there on, down and up again, it takes the clear-layer step with the cell's
 *   atrans, bbd and bbu.  The branch tests are the reference's, literally: odtot < 0.06, od <= 0.06.
 *   flux(level) = fluxfac * sum over B of delwave(B) * 0.5 * sum over the g-points of B of rad (the derivatives alike); the order of
 *   these sums is the library's.  hr(l) = heatfac * (net(l) - net(l+1)) / (plev(l) - plev(l+1)), net = up - down, as
 *   rrtmg_lw_hip_adjust_tsfc defines it.
 * uflx, dflx and hr are required; uflxc, dflxc and hrc are all set or all NULL; dplankbnd_dt, duflx_dt and duflxc_dt are needed with
 * idrv = 1 only and not touched otherwise.  A NULL output is neither formed nor touched.
 * RRTMG_LW_HIP_EARG, with a text that names the argument and before anything is written: cloud other than 0, 1, 2; idrv other than 0,
 * 1; a missing required array; a half-given clear-sky triple; the dimension limits of the other entries; an output that shares a byte
 * with an input the call reads or with another output.  There are no physics errors: a non-finite input gives non-finite output in its
 * own column only.
 * rrtmg_lw_hip_solve_device: DEVICE pointers; the device is that of tau; it enqueues on `stream` and does not synchronise.  The entry
 * lock, no graph replay, no combining.  Column batches of rrtmg_lw_hip_effective_batch(nlay); per batch k_solve - one thread per (column,
 * band), the band's g-points four at a time in registers, the upward sweep reading tau and fracs again instead of keeping per-level values -
 * and k_solve_flux, one thread per column.  The only workspace is the per-band partial sums, 16 x (nlay + 1) x 8 B per column of a
 * batch for each of upward, downward (cloud = 0), their clear-sky pair (cloud != 0) and the derivatives (idrv = 1); counted in
 * rrtmg_lw_hip_workspace_bytes.  A column's results do not depend on its neighbours or on the batch size, to the last bit.
 * rrtmg_lw_hip_solve: HOST pointers, the first device; staged in column batches (rrtmg_lw_hip_set_batch, at most 16 384) through the
 * host-entry staging buffer, as rrtmg_lw_hip_cloud_optics does.  Synchronises.
 * Not offered: rtrnmr (maximum-random overlap), array forms and views, _r4, spectral outputs, fan-out over several devices, graph
 * replay. */
int rrtmg_lw_hip_solve(int ncol, int nlay, int cloud, int idrv,
    const double *plev, const double *emis,
    const double *tau, const double *fracs,
    const double *planklay, const double *planklev, const double *plankbnd, const double *dplankbnd_dt,
    const double *cldfr, const double *odcld, const unsigned *submask,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt);
int rrtmg_lw_hip_solve_device(int ncol, int nlay, int cloud, int idrv,
    const double *plev, const double *emis,
    const double *tau, const double *fracs,
    const double *planklay, const double *planklev, const double *plankbnd, const double *dplankbnd_dt,
    const double *cldfr, const double *odcld, const unsigned *submask,
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc,
    double *duflx_dt, double *duflxc_dt, void *stream);

/* ---- Host arrays of a host built with 4-byte reals ("_r4") ----------------------------------------------------------------------------
 * A host model that carries RRTMG_LW at the default real kind (no -r8) owns float arrays.  These four entries take them as they are:
 * HOST pointers, every floating-point array of the call - inputs and outputs, alpha too - `float`.  Layout, argument order, the in/out
 * behaviour of icld and irng, flags, NULL rules, error codes and error texts are those of the float64 entry each is named after.
 * Results: what the float64 entry returns on the same values widened to double, each output rounded to nearest ((float)x), bit for bit.
 * The solver works in float64 as always; the float64 entries are what they were.
 *   rrtmg_lw_hip_run_nomcica_r4        as rrtmg_lw_hip_run_nomcica.  Takes the entry lock: a small call does NOT join the combining of
 *                                      concurrent small calls (like the spectral entries).
 *   rrtmg_lw_hip_run_mcica_r4          as rrtmg_lw_hip_run_mcica (explicit (140,ncol,nlay) sub-column arrays).
 *   rrtmg_lw_hip_run_mcica_subcol_r4   as rrtmg_lw_hip_run_mcica_subcol (fused generator + solver); no combining either.
 *   rrtmg_lw_hip_adjust_tsfc_r4        as rrtmg_lw_hip_adjust_tsfc: the arithmetic in float64 on the widened values, as
 *                                      rrtmg_lw_hip_adjust_tsfc_device_as defines it for real_bytes = 4.
 * All four take the entry lock, split their columns over the devices of rrtmg_lw_hip_init_devices and run through the pipeline of the
 * float64 host entries with 4-byte elements: a row that holds one 4-byte pattern for all columns of a batch does not travel (its widened
 * value is filled in on the device), every other row crosses as float32 - from where it lies when the array is registered, packed by the
 * host threads when it is pageable - into a float32 landing area of the staging set and is widened there by one kernel per batch; the
 * active outputs are rounded into the landing area by one kernel per batch and leave as float32.  With inflglw >= 1 the band sum of
 * taucld is formed on the host in float64 on the widened values, in the reference's band order.  rrtmg_lw_hip_host_register /
 * _is_registered / _static / _changed take byte ranges: pass 4 bytes per element.  An address declared static and later passed with the
 * other element type is scanned anew.
 * Workspace: the landing area - per column of a batch 4 bytes for every input value and every active output value - beside the float64
 * staging arrays (8 bytes each), four staging sets; counted in rrtmg_lw_hip_workspace_bytes.
 * Out of scope: the spectral outputs, the chunk queue, the prepared-column entries, the gas-optics entries, the stand-alone generator and
 * get_alpha (the Fortran layer covers those two by conversion), and any array layout other than the reference's. */
int rrtmg_lw_hip_run_nomcica_r4(
    int ncol, int nlay, int *icld, int idrv,
    const float *play, const float *plev, const float *tlay, const float *tlev, const float *tsfc,
    const float *h2ovmr, const float *o3vmr, const float *co2vmr, const float *ch4vmr, const float *n2ovmr,
    const float *o2vmr, const float *cfc11vmr, const float *cfc12vmr, const float *cfc22vmr,
    const float *ccl4vmr, const float *emis, int inflglw, int iceflglw, int liqflglw,
    const float *cldfr, const float *taucld, const float *cicewp, const float *cliqwp,
    const float *reice, const float *reliq, const float *tauaer,
    float *uflx, float *dflx, float *hr, float *uflxc, float *dflxc, float *hrc,
    float *duflx_dt, float *duflxc_dt);
int rrtmg_lw_hip_run_mcica_r4(
    int ncol, int nlay, int *icld, int idrv,
    const float *play, const float *plev, const float *tlay, const float *tlev, const float *tsfc,
    const float *h2ovmr, const float *o3vmr, const float *co2vmr, const float *ch4vmr, const float *n2ovmr,
    const float *o2vmr, const float *cfc11vmr, const float *cfc12vmr, const float *cfc22vmr,
    const float *ccl4vmr, const float *emis, int inflglw, int iceflglw, int liqflglw,
    const float *cldfmcl, const float *taucmcl, const float *ciwpmcl, const float *clwpmcl,
    const float *reicmcl, const float *relqmcl, const float *tauaer,
    float *uflx, float *dflx, float *hr, float *uflxc, float *dflxc, float *hrc,
    float *duflx_dt, float *duflxc_dt);
int rrtmg_lw_hip_run_mcica_subcol_r4(
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    const float *play, const float *plev, const float *tlay, const float *tlev, const float *tsfc,
    const float *h2ovmr, const float *o3vmr, const float *co2vmr, const float *ch4vmr, const float *n2ovmr,
    const float *o2vmr, const float *cfc11vmr, const float *cfc12vmr, const float *cfc22vmr,
    const float *ccl4vmr, const float *emis, int inflglw, int iceflglw, int liqflglw,
    const float *cldfr, const float *taucld, const float *cicewp, const float *cliqwp,
    const float *reice, const float *reliq, const float *alpha, const float *tauaer,
    float *uflx, float *dflx, float *hr, float *uflxc, float *dflxc, float *hrc,
    float *duflx_dt, float *duflxc_dt);
int rrtmg_lw_hip_adjust_tsfc_r4(int ncol, int nlay, const float *plev, const float *dtsfc,
    const float *uflx, const float *dflx, const float *duflx_dt,
    const float *uflxc, const float *dflxc, const float *duflxc_dt,
    float *uflx_adj, float *hr_adj, float *uflxc_adj, float *hrc_adj);

/* PMC calibration: one kernel that reads `bytes` and writes `bytes` with 16 B per lane (known HBM traffic), so that a
 * rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE pass can fix the counters' unit and scale in the same session. */
int rrtmg_lw_hip_calibrate_stream(long long bytes);

#ifdef __cplusplus
}
#endif
#endif
