// CDNA4 (gfx950) kernels of the RRTMG_LW hot path.  Written for MI355X only.
//
// Mapping (DESIGN.md "Kernels"): the caller's arrays are (ncol, nlay) with the COLUMN index fastest
// (reference: src/rrtmg_lw_rad.nomcica.f90:219-276), so lanes = consecutive columns makes every load and
// store of profile, scratch and flux data a full-width coalesced access.  The work is split where the
// reference's data dependence allows it:
//
//   k_colsort  cloudy batches: the order in which the later kernels take the columns - by cloud top within windows of 256, where that
//              makes the sweeps' 64-column blocks alike (workspace arrays by position, the caller's arrays by column)   1 workgroup / window
//   k_colprep  per-column scalars: laytrop, precipitable water -> diffusivity secants, surface Planck
//              terms                                                    1 thread / column
//   k_cloudscan / k_cloudlay   cldprop, cloud optical depth per spectral band: the one quantity cldprop carries from layer
//              to layer per column, then the per-layer physics        1 thread / column, 1 thread / (column, layer)
//   k_cloudmc  cldprmc + the cloud set-up of rtrnmc (McICA)             1 thread / (column, layer)
//   k_blocksort  the 64-column blocks of a batch ordered by their highest cloudy layer, one hand-off level per group of blocks
//                                                                       1 workgroup / batch
//   k_layer    everything that is LOCAL to a layer: inatm + setcoef + taumol for all bands (the bands' absorption tables staged
//              in LDS, several bands per pass, for the 256 columns of a workgroup, which share the layer), then for each cell the
//              decision rtrn takes on its optical depth (series / table index) as a 4-byte code
//                                                                       1 thread / (column, layer)
//   k_sweepc / k_sweepz   the only vertically serial part: the down/up recurrences of rtrn / rtrnmr / rtrnmc over the cell codes
//              (transmittance table, the bands' Planck integrals and fractions in LDS); k_sweepc above the hand-off level of the
//              wave's block group and for cloud-free calls (1 thread / (column, band)), k_sweepz in the cloud zone (1 thread /
//              (column, quad)); a workgroup = the bands of one group, flux partials added over the group in LDS
//   k_flux     group partials -> fluxes, net fluxes, heating rates           1 thread / (column, chunk of levels)
//   k_subcol_* McICA sub-column generator (bit masks), k_alpha           see the section below
//   k_cloudcover  the generator's masks counted: total, cumulative and per-layer cloud cover, the mask itself    1 thread / column
//   k_cloudoptics_col / k_cloudoptics   cldprop / cldprmc as OUTPUTS: band optical depths before the secant, ncbands, secdiff    1 thread / column, / (column, layer)
//   k_solve / k_solve_flux   rtrn / rtrnmc on the CALLER's optical depths and sources, float64 tables, no cell codes (rrtmg_lw_hip_solve*)
//                                                                       1 thread / (column, band), 1 thread / column
//
// Reference lines are cited per routine.  No CPU fallback exists anywhere in this file.
#include <hip/hip_runtime.h>
#include "kissjump.hpp"

// ------------------------------------------------------------------------------------------------
// Build switches.  -DRRLW_G256 is the product's 256-g-point configuration and -DRRLW_TUNE the tuning build (the benchmark's kernels only:
// a one-minute compile).  What remains beside them are plain numbers with one use each (block sizes, waves-per-SIMD tables: same results,
// other speed) and two instruments that have tools (RRLW_LAYER_STAMPS, RRLW_DBG_DUMP); the shipped libraries are built with none of
// them.  What a library was built with is recorded in its build-flags word (rrtmg_lw_hip_build_flags): bit 0 tuning, bit 3 G256, bit 4
// geometry.  Bits 1 and 2 (knock-out, numerics variant) are reserved: the switches that set them - alternate code paths of experiments
// that were run and lost - are retired, with their results under profiles/ (profiles/switch_retirement.md lists them).
// ------------------------------------------------------------------------------------------------
#ifdef RRLW_TUNE
#define RRLW_BF_TUNE 1u
#else
#define RRLW_BF_TUNE 0u
#endif
#ifdef RRLW_G256
#define RRLW_BF_G256 8u
#else
#define RRLW_BF_G256 0u
#endif
// kernel-geometry switches given on the command line (same results, other speed)
#if defined(RRLW_LAYER_BLOCK) || defined(RRLW_STAGE_DOUBLES) || defined(RRLW_LAYER_WAVES) || defined(RRLW_LOAD_CHUNK) || defined(RRLW_MINOR_WIN) || \
    defined(RRLW_COLSORT_WIN) || defined(RRLW_SWEEPC_P0) || defined(RRLW_SWEEPC_P2D) || defined(RRLW_SWEEPC_WAVES_CAP) || defined(RRLW_SWEEPC_CODES) || \
    defined(RRLW_SWEEPZ_WAVES_G1) || defined(RRLW_SWEEPZ_WAVES_IDRV) || defined(RRLW_LAYER_STAMPS) || \
    defined(RRLW_DBG_DUMP)      /* (driver.hip: one more entry, rrtmg_lw_hip_debug_scratch - reads k_layer's cell codes back; tuning builds only) */
#define RRLW_BF_GEOMETRY 16u
#else
#define RRLW_BF_GEOMETRY 0u
#endif

#include <algorithm>
#include <type_traits>
#include <utility>

#include "tables.hpp"

namespace rrlw {

constexpr unsigned BUILD_FLAGS = RRLW_BF_TUNE | RRLW_BF_G256 | RRLW_BF_GEOMETRY;

// ------------------------------------------------------------------------------------------------
// device-side views
// ------------------------------------------------------------------------------------------------
struct DevTables {
    const double *ktab;
    const double *stat;
    BandLayout band[NBND];
    StaticLayout sl;
    double absice0[2], abscld1, absliq0;
    double delwave[NBND];
    double refrat[NBND][6];
    double heatfac, fluxfac, oneminus, bpade;
};

// setcoef quantities of one (layer, column) - indices into LayerCoef::f
enum Field {
    F_FAC00, F_FAC01, F_FAC10, F_FAC11,
    F_COLH2O, F_COLCO2, F_COLO3, F_COLN2O, F_COLCO, F_COLCH4, F_COLO2, F_COLBRD,
    F_COLDRY, F_SELFFAC, F_SELFFRAC, F_FORFAC, F_FORFRAC, F_MINORFRAC, F_SCALEMINOR, F_SCALEMINORN2,
    F_PAVEL, F_WX1, F_WX2, F_WX3, F_WX4,
    NFIELD
};
// per-column doubles, each [ncolb]
enum PerCol { PC_PLANKBND = 0, PC_DPLANKBND = 16, PC_SECDIFF = 32, NPERCOL = 48 };
// per-cell transmittance codes handed from k_layer to the sweeps, each [NQUAD][nlay][ncolb][4] (see cell_code):
// gas optical depth of every cell, total (gas + cloud) optical depth of the cells of cloudy layers
enum Scr { S_CODE, S_CODET, NSCR };
// per-band partial fluxes, each [band][level][column] of {total-sky, clear-sky}: downward, upward, d(upward)/dT
struct alignas(16) Part2 { double a, b; };

// the per-cell codes handed from k_layer to the sweeps (all arithmetic stays float64): in registers and in memory a float (scr_t,
// cell_code), four cells (a quad) per record.  (24- and 16-bit records, which kept the table index whole and rounded the series-branch
// optical depth to 18 / 11 mantissa bits, were measured in round 3 and lost: profiles/round3_code_bits.md.)
typedef float scr_t;
constexpr int CODE_WORDS = 4;                    // 32-bit words per quad record
constexpr int CODE_BYTES = 4 * CODE_WORDS;

struct Workspace {
    int ncolb;          // column stride (batch capacity)
    int nlay;
    double *percol;     // [NPERCOL][ncolb]
    int *laytrop;       // [ncolb]
    int *ncbands;       // [ncolb]
    double *odcld;      // [16][nlay][ncolb]   secdiff(ib) * taucloud
    double *efcl;       // [16][nlay][ncolb]   rtrn: (1 - exp(-odcld)) * cldfrac
    int *cflag;         // [nlay+2][ncolb]  bit0 icldlyr, bit1 istcldd (first cloudy level of a block, downward sweep), bit2 istcld (upward); cflag[0] bit3 = column has cloud
    double2 *ovl;       // rtrnmr's overlap factors of the cloudy levels: [2: down, up][nlay+1][3][ncolb] {facclr1, faccld1} {faccmb1, faccmb2} {facclr2, faccld2}
    // Where the clouds end.  A sweep wave works on a BLOCK of 64 consecutive columns; above the highest cloud of its block every layer is
    // clear in every column and the cheap clear-sky sweep (k_sweepc) serves.  k_cloudscan / k_cloudmc record the top per block, k_blocksort
    // orders the blocks by it (deepest first) and gives every group of SORT_GROUP consecutive sorted blocks ONE hand-off level, the
    // group's highest top: a sweep workgroup takes 1, 2, 3, 4, 6 or 12 consecutive sorted blocks of one group, whatever the kernel.
    int *btop;          // [nblk]  highest layer that holds cloud in any column of the block (0: none)
    int *order;         // [nslot] sorted position -> block (positions past the last block: nblk, i.e. columns past the end)
    int *hgrp;          // [nslot / SORT_GROUP] hand-off level of the group
    int *hblk;          // [nblk]  hand-off level of the block's group (k_flux)
    int *bbot;          // [nblk]  lowest layer that holds cloud in any column of the block (nlay + 1: none)
    int *hbot;          // [nslot / SORT_GROUP] lowest cloudy layer of the group: below it the cloud-zone sweep runs its clear-sky body without the cloudy-level inputs
    double *hand;       // [5][NQUAD][ncolb][4] radiances handed from sweep to sweep at the block's hand-off level: 0 downward (k_sweepc<.,1> -> k_sweepz), 1 / 2 upward
                        // total / clear (k_sweepz -> k_sweepc<.,2>), 3 / 4 their d/dT (idrv = 1)
    unsigned *scr[NSCR];   // [NQUAD][nlay][ncolb] quad records of CODE_WORDS words
    unsigned *fw;       // [NFW][nlay][ncolb]   binary-key bands: Planck-fraction interpolation (js << 28 | 28-bit fs)
    // k_sweepc's partials, summed over the bands of a GROUP (bands with the same number of quads, swept by one workgroup and added in
    // LDS): [NGROUP_MAX][nlay+1][ncolb].  gdn1 / gup1: 8 bytes where the clear-sky stream equals the total one (downward at and above the
    // batch's highest cloud, both directions of a cloud-free call); gup / gdp {total, clear}: upward above the clouds, d(flux)/dT
    double *gdn1, *gup1;
    Part2 *gup, *gdp, *gdn;     // gdn {total, clear}: downward inside the cloud zone (k_sweepz)
    // column stride of those slabs: ncolb - or, for a batch too small to fill the chip, whose bands are swept ONE per workgroup and leave a
    // slab each (SweepArgs::split), the batch's own width (the slabs' memory then holds sixteen narrow slabs instead of four wide ones)
    int pcb;
    int *err;           // [1] first physics error code
    // McICA (rtrnmc): per-g-point cloud terms, written by k_cloudmc
    double *odg;        // [NQUAD][nlay][ncolb][4]     secdiff(band) * taucmc(g)
    float *cfef;        // [NQUAD][nlay][ncolb][8]     {cldfmc(g) x4, efclfrac(g) x4}
    unsigned *mask;     // [MASK_WORDS][nlay][mask_stride]      sub-column cloud mask of ALL columns of the call (indexed by the global
    size_t mask_stride; //                             column mask_col0 + col0 + col), bit k of word w = sub-column 32 w + k
    size_t mask_col0;
    // The order in which the batch's columns are taken (k_colsort): position (slot) -> column of the batch, or null = as they come.  Every
    // workspace array above is indexed by SLOT, the caller's arrays by COLUMN (pcol).
    // k_layer's (window, layer) pairs whose cells do not fit the narrow staging window, left by the narrow launch for the wide one:
    // {count, unused, pair ..}; null: no wide launch follows (every workgroup keeps the narrow window)
    int *wide;          // [2 + windows * nlay]
    int *perm;          // [ncolb rounded up to whole windows]
    int *wsort;         // [windows] 1: the window's columns are taken in another order than they lie
    // ... and for such windows the rows the sweeps read of the caller's arrays at EVERY level - layer and interface temperatures, cloud
    // fraction - once more in position order (k_colsort): [nlay | nlay+1 | nlay][ncolb]
    double *tlayc, *tlevc, *cldfc;
};
#ifndef RRLW_COLSORT_WIN
#define RRLW_COLSORT_WIN 256
#endif
constexpr int COLSORT_WIN = RRLW_COLSORT_WIN;       // columns of a k_colsort window
// (a wavefront's positions lie in ONE window - 64 consecutive positions from a multiple of 64, or all the last column's: the window's flag is
// a scalar load, and a window that kept its order does not wait for its `perm` entries, a cold vector load at the head of every kernel)
__device__ __forceinline__ bool pmoved(const Workspace &W, int slot) { return W.perm && W.wsort[__builtin_amdgcn_readfirstlane(slot) / COLSORT_WIN] != 0; }
__device__ __forceinline__ int pcol(const Workspace &W, int slot)
{
    if (!W.perm) return slot;
    const int moved = W.wsort[__builtin_amdgcn_readfirstlane(slot) / COLSORT_WIN];     // (uniform address: a scalar load)
    return moved ? W.perm[slot] : slot;
}
// One value of a row of the caller's (column-fastest) arrays: wave-uniform row pointer in a buffer descriptor, the lane's column as a 32-bit
// byte offset - the column is a loaded value (pcol), and as part of a 64-bit address it would cost every load its own address arithmetic.
__device__ __forceinline__ double col_load(const double *row, unsigned off8)
{
    typedef unsigned int u32x2c __attribute__((ext_vector_type(2)));
    const u32x2c v = __builtin_amdgcn_raw_buffer_load_b64(__builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(row), 0, 0x7ffffff0, 0x00020000), (int)off8, 0, 0);
    double r;
    __builtin_memcpy(&r, &v, 8);
    return r;
}

// GCM-interface inputs (device pointers, column stride = ncol_total), reference src/rrtmg_lw_rad.nomcica.f90:219-276
struct GcmIn {
    const double *play, *plev, *tlay, *tlev, *tsfc, *h2ovmr, *o3vmr, *co2vmr, *ch4vmr, *n2ovmr, *o2vmr;
    const double *cfc11vmr, *cfc12vmr, *cfc22vmr, *ccl4vmr, *emis;
    const double *cldfr, *taucld, *cicewp, *cliqwp, *reice, *reliq, *tauaer;
    const double *tauctot = nullptr;    // (ncol,nlay), optional: the sum of taucld over the bands where the caller has formed it (host entry, inflglw >= 1); taucld is null then
};
// prepared-column inputs (device pointers, column stride = ncol_total), reference src/rrtmg_lw.1col.f90:497-580
struct ColIn {
    const double *pavel, *tavel, *pz, *tz, *tbound, *semiss, *coldry, *wkl, *wbrodl, *wx, *pwvcm;
    const double *cldfrac, *tauc, *ciwp, *clwp, *rei, *rel, *taua;
};
// McICA cloud inputs (device pointers), reference src/rrtmg_lw_rad.f90:267-298
struct McIn {
    const double *cldfmcl, *taucmcl, *ciwpmcl, *clwpmcl;   // (140, ncol_total, nlay)
    const double *reicmcl, *relqmcl;                       // (ncol_total, nlay)
};
struct FluxOut {
    double *uflx, *dflx, *hr, *uflxc, *dflxc, *hrc, *duflx_dt, *duflxc_dt;   // stride ncol_total
    double *fnet, *fnetc;                                                     // optional (column entry)
    double *uflxs, *dflxs, *uflxcs, *dflxcs;                                  // optional spectral outputs (ncol_total, nlay+1, 16): written by the sweeps (SweepArgs)
    double *uflx_var, *dflx_var, *hr_var;                                     // optional, each on its own: sample variances of uflx, dflx, hr (k_flux_var), their shapes
};
// Outputs of the gas-optics entries (k_optics), device pointers, column stride = ncol_total, g-point or band index last:
// taug, fracs (ncol_total, nlay, NGPT); planklay (.., nlay, 16); planklev (.., nlay+1, 16); plankbnd, dplankbnd (.., 16).
// taug and fracs are required, the others optional (null: not stored); dplankbnd is stored only with idrv = 1.
struct OptOut {
    double *taug = nullptr, *fracs = nullptr, *planklay = nullptr, *planklev = nullptr, *plankbnd = nullptr, *dplankbnd = nullptr;
};

enum ErrCode { E_NONE = 0, E_ICE_SMALL = 1, E_ICE_BOUNDS = 2, E_ICE_GEN_BOUNDS = 3, E_LIQ_BOUNDS = 4, E_BAD_FLAG = 5,
               E_MC_INFLAG1 = 6, E_KISS_PMID = 7 };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// a / b for normal, finite operands in k_layer: hardware reciprocal seed (2^-24), ONE Newton step (2^-48), one residual correction
// q + (a - b q) r, whose error is the product of the two (6 VALU operations in one dependency chain instead of the ~13 of the IEEE
// sequence with its scale / fix-up steps; a third of k_layer's VALU instructions were divisions).  The quotient is within an ulp of
// the correctly rounded one; where it feeds an index (`int(...)`, the 1e-4-quantised transmittance table) a different index needs the
// exact quotient to sit within ~1e-16 of a boundary: tools/divtest.hip finds 0 quotients and 0 table indices different from the IEEE
// division in 2.1e9 operands, with one Newton step as with two (profiles/round2_divtest.txt; round 3 made one the default: -0.3 ms).
__device__ __forceinline__ double fdiv(double a, double b)
{
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);
    const double q = a * r;
    return fma(fma(-b, q, a), r, q);
}

// ------------------------------------------------------------------------------------------------
// k_colsort : the order in which every later kernel takes the batch's columns.  The sweeps decide per wavefront - 64 consecutive positions -
//             where the clouds end (Workspace::btop): one deep tower among 64 shallow columns sends all of them through the cloud-zone sweep
//             up to its top, and one cloudy column among clear ones likewise.  Within each window of COLSORT_WIN consecutive columns (the
//             columns of ONE k_layer workgroup, so that what a workgroup reads of the caller's arrays is the same few cache lines in any
//             order) the columns are ordered by their highest cloudy layer, deepest first, equal tops in column order - a homogeneous window
//             keeps its order.  Results do not depend on the order (a column does not depend on its neighbours); the reference has no
//             counterpart: it takes the columns one by one (src/rrtmg_lw_rad.nomcica.f90:472).
// ------------------------------------------------------------------------------------------------
// A window is reordered only where that pays: reading the caller's arrays out of order costs every kernel something (eight-byte accesses
// spread over the window's cache lines instead of consecutive ones), so the order is taken when it removes at least `min_gain` block-levels
// from the cloud zone - the sum over the window's four 64-column blocks of the block's highest cloudy layer, as the columns lie against
// sorted - and the window keeps its order otherwise (a homogeneous deck, a tower system that fills whole blocks).  A block that holds no
// cloud at all once sorted and did as the columns lie is worth more than its top: where its group of sorted blocks is cloud-free too it
// leaves the cloudy launches altogether for the one-stream sweep of a cloud-free call (SweepArgs::cfree).  `clear_bonus` block-levels are
// added to the gain for each such block (driver.hip: g_colsort_clear, a share of nlay).
constexpr int COLSORT_TY = 4;       // threads per column: the walk over the layers and the copy of the rows in four parts
template <bool GCM>
__global__ __launch_bounds__(COLSORT_WIN * COLSORT_TY) void k_colsort(Workspace W, GcmIn g, ColIn c, int ncol, int col0, int nct, int min_gain, int clear_bonus)
{
    constexpr int NB = COLSORT_WIN / 64;
    __shared__ int s_key[COLSORT_WIN], s_perm[COLSORT_WIN], s_top[COLSORT_TY][COLSORT_WIN];
    __shared__ int s_nat[NB], s_srt[NB];
    const int t = threadIdx.x, ty = threadIdx.y, w0 = blockIdx.x * COLSORT_WIN, col = w0 + t;
    const int nlay = W.nlay;
    int top = -1;                                   // a position past the last column: after everything
    if (col < ncol) {
        const double *cf = (GCM ? g.cldfr : c.cldfrac) + (size_t)col0 + col;
        const int per = (nlay + COLSORT_TY - 1) / COLSORT_TY, l0 = ty * per + 1, l1 = min(nlay, l0 + per - 1);
        top = 0;
#pragma unroll 8
        for (int lay = l0; lay <= l1; lay++) { if (cf[(size_t)nct * (lay - 1)] >= 1.e-6) top = lay; }      // (k_cloudscan's `cloudy`)
    }
    s_top[ty][t] = top;
    __syncthreads();
    int rank = 0;
    if (ty == 0) {
#pragma unroll
        for (int k = 1; k < COLSORT_TY; k++) top = max(top, s_top[k][t]);
        s_key[t] = (nlay - top) * COLSORT_WIN + t;  // deepest first, then column order
        int mx = max(top, 0);                       // the block's top as the columns lie: a wave = 64 consecutive columns
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
        if ((t & 63) == 0) s_nat[t >> 6] = mx;
    }
    __syncthreads();
    if (ty == 0) {
        const int key = s_key[t];
#pragma unroll 8
        for (int i = 0; i < COLSORT_WIN; i++) rank += s_key[i] < key ? 1 : 0;
        if ((rank & 63) == 0) s_srt[rank >> 6] = max(top, 0);      // ... and sorted: the first of every 64 is the deepest
    }
    __syncthreads();
    int gain = 0;
#pragma unroll
    for (int b = 0; b < NB; b++) gain += s_nat[b] - s_srt[b] + ((s_srt[b] == 0 && s_nat[b] != 0) ? clear_bonus : 0);
    const bool keep = gain * 4 < min_gain * NB;     // (uniform over the workgroup; min_gain is quoted for four blocks)
    if (ty == 0) {
        if (keep) rank = t;
        if (t == 0) W.wsort[blockIdx.x] = keep ? 0 : 1;
        W.perm[w0 + rank] = col;
        s_perm[rank] = col;
    }
    if (keep) return;
    // A reordered window: the rows of the caller's arrays that the sweeps read at EVERY level - layer and interface temperatures, cloud
    // fraction - once more in position order (Workspace::tlayc ..), read through the new order, written consecutively.  (Out-of-order
    // eight-byte reads cost the sweeps 5 ms per 1e6 deep-cloud columns where they recurred per level and band.)
    if constexpr (GCM) {
        __syncthreads();
        const int slot = w0 + t;
        if (slot < ncol) {
            const size_t g0 = (size_t)col0 + s_perm[t];
#pragma unroll 4
            for (int lev = ty; lev <= nlay; lev += COLSORT_TY) {         // level 0 .. nlay; layer lev + 1 for the two layer arrays
                const size_t gi = g0 + (size_t)nct * lev, o = (size_t)lev * W.ncolb + slot;
                W.tlevc[o] = g.tlev[gi];
                if (lev < nlay) { W.tlayc[o] = g.tlay[gi]; W.cldfc[o] = g.cldfr[gi]; }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_colprep : the per-column reductions of inatm (src/rrtmg_lw_rad.nomcica.f90:785-870: amttl, wvttl ->
//             pwvcm), setcoef's laytrop count and surface Planck terms (src/rrtmg_lw_setcoef.f90:173-215,
//             :312-313) and the diffusivity secants (src/rrtmg_lw_rtrn.f90:265-288).
// ------------------------------------------------------------------------------------------------
template <bool GCM>
__global__ __launch_bounds__(256) void k_colprep(DevTables T, Workspace W, GcmIn g, ColIn c, int ncol, int col0, int nct, int idrv, int istart, int init_cloud)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncol) return;
    const size_t gc = (size_t)col0 + pcol(W, col);
    const int nlay = W.nlay;
    const double *S = T.stat;
    const double *totplnk = S + T.sl.totplnk, *totplnkd = S + T.sl.totplnkderiv;
    const double *totplk16 = S + T.sl.totplk16, *totplk16d = S + T.sl.totplk16deriv;
    const double amd = 28.9660, amw = 18.0160, avogad = 6.02214199e+23, grav = 9.8066;

    const double tbound = GCM ? g.tsfc[gc] : c.tbound[gc];
    const double pz0 = GCM ? g.plev[gc] : c.pz[gc];
    const int indbound = clampi((int)(tbound - 159.), 1, 180);
    const double tbndfrac = tbound - 159. - (double)indbound;
#pragma unroll
    for (int b = 0; b < NBND; b++) {
        const double semiss = GCM ? g.emis[gc + (size_t)nct * b] : c.semiss[gc + (size_t)nct * b];
        const double *tp = (b == 15 && istart == 16) ? totplk16 : totplnk + 181 * b;        // :233-242
        const double *td = (b == 15 && istart == 16) ? totplk16d : totplnkd + 181 * b;
        const double pb = semiss * (tp[indbound - 1] + tbndfrac * (tp[indbound] - tp[indbound - 1]));
        double dpb = 0.0;
        if (idrv == 1) dpb = semiss * (td[indbound - 1] + tbndfrac * (td[indbound] - td[indbound - 1]));
        W.percol[(size_t)(PC_PLANKBND + b) * W.ncolb + col] = pb;
        W.percol[(size_t)(PC_DPLANKBND + b) * W.ncolb + col] = dpb;
    }
    double amttl = 0.0, wvttl = 0.0, pzlo = pz0;
    int laytrop = 0;
    // (a thread walks its column alone: unrolled, the loads of eight layers are in flight together instead of one round trip per layer -
    // on the critical path of every call that is a single batch)
#pragma unroll 8
    for (int lay = 1; lay <= nlay; lay++) {
        const size_t gi = gc + (size_t)nct * (lay - 1);
        const double pavel = GCM ? g.play[gi] : c.pavel[gi];
        if (!(log(pavel) <= 4.56)) laytrop++;
        if (GCM) {
            const double w1v = g.h2ovmr[gi];
            const double pzl = g.plev[gc + (size_t)nct * lay];
            const double amm = (1. - w1v) * amd + w1v * amw;
            const double coldry = (pzlo - pzl) * 1.e3 * avogad / (1.e2 * grav * amm * (1. + w1v));
            pzlo = pzl;
            const double w1 = coldry * w1v;
            amttl = amttl + coldry + w1;
            wvttl = wvttl + w1;
        }
    }
    W.laytrop[col] = laytrop;
    double pwvcm;
    if (GCM) {
        const double wvsh = (amw * wvttl) / (amd * amttl);
        pwvcm = wvsh * (1.e3 * pz0) / (1.e2 * grav);
    } else {
        pwvcm = c.pwvcm[gc];
    }
    const double a0[16] = {1.66, 1.55, 1.58, 1.66, 1.54, 1.454, 1.89, 1.33, 1.668, 1.66, 1.66, 1.66, 1.66, 1.66, 1.66, 1.66};
    const double a1[16] = {0.00, 0.25, 0.22, 0.00, 0.13, 0.446, -0.10, 0.40, -0.006, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00};
    const double a2[16] = {0.00, -12.0, -11.7, 0.00, -0.72, -0.243, 0.19, -0.062, 0.414, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00};
#pragma unroll
    for (int b = 0; b < NBND; b++) {
        double sd = 1.66;
        if (!(b == 0 || b == 3 || b >= 9)) {
            sd = a0[b] + a1[b] * exp(a2[b] * pwvcm);
            if (sd > 1.80) sd = 1.80;
            if (sd < 1.50) sd = 1.50;
        }
        W.percol[(size_t)(PC_SECDIFF + b) * W.ncolb + col] = sd;
    }
    // (the cloud-free defaults, and the block tops k_cloudmc raises with atomics; k_cloudscan writes all of these itself and may run BESIDE
    // this kernel - run_prep - so they are left alone for it: init_cloud = 0)
    if (init_cloud) {
        W.ncbands[col] = 1;
        W.cflag[col] = 0;
        if ((col & 63) == 0) { W.btop[col >> 6] = 0; W.bbot[col >> 6] = nlay + 1; }
    }
}

// ------------------------------------------------------------------------------------------------
// k_cloud : cldprop (src/rrtmg_lw_cldprop.f90:50-295), cloud optical depth along the diffusivity
//           angle (rtrn :321-334 / rtrnmr :333-343).  mode 1 = rtrn, 2 = rtrnmr.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int icb_map(int ib, int ind)   // cldprop :167-169 (1-based ib)
{
    if (ind == 0) return 1;
    if (ind == 2) return ib;
    return ib <= 2 ? ib : (ib <= 5 ? 3 : (ib <= 8 ? 4 : 5));
}

// cldprop carries two things from layer to layer of a column (src/rrtmg_lw_cldprop.f90:173-293): `ncbands`, assigned by the layers that
// hold ice or liquid water and left alone by the others, and nothing else that matters (iceind / liqind are reassigned before every
// use).  k_cloudscan walks a column once and records the band count in effect at each layer; k_cloudlay then does the per-layer physics
// for all (column, layer) pairs in parallel - the serial kernel this replaces kept one wave per 64 columns busy for 0.8 ms per batch.
__device__ __forceinline__ bool cloud_layer_enters(double cf, double cwp, double tauctot)      // cldprop :186
{
    const double cldmin = 1.e-20;
    return cf >= cldmin && (cwp >= cldmin || tauctot >= cldmin);
}
template <bool GCM>
__device__ __forceinline__ double cloud_tauctot(const GcmIn &g, const ColIn &c, size_t gc, size_t gi, int nct, int lay)
{
    if constexpr (GCM) { if (g.tauctot) return g.tauctot[gi]; }
    double tauctot = 0.0;                               // taucld (16,ncol,nlay) | tauc (ncol,16,nlayers)
    for (int ib = 0; ib < NBND; ib++)
        tauctot = tauctot + (GCM ? g.taucld[ib + (size_t)NBND * gi] : c.tauc[gc + (size_t)nct * (ib + (size_t)NBND * (lay - 1))]);
    return tauctot;
}

// Maximum-random overlap factors of ONE cloudy level, src/rrtmg_lw_rtrnmr.f90:347-506 (upward loop :347-425, downward loop :427-506;
// the two loops are mirror images).  cl = cloud fraction of the level, cn = of the next level in sweep direction, cp = of the previous
// one (read only when that level is cloudy, i.e. !first), last = the level is the last of the sweep.  rat1 / rat2 carry from cloudy
// level to cloudy level as in the reference.  faccmb1/2, which the reference reads uninitialised when first, are ZERO.
struct OvlFac { double clr1, cld1, cmb1, cmb2, clr2, cld2; bool rat1, rat2; };     // rat1 / rat2 (0 or 1 in the reference): carried to the next cloudy level
__device__ __forceinline__ OvlFac mr_step(double cl, double cn, double cp, bool first, bool last, bool brat1, bool brat2)
{
    const double rat1 = brat1 ? 1. : 0., rat2 = brat2 ? 1. : 0.;
    // (everything by value: carried state behind references ends up in scratch memory).  Of the reference's seven ways through this
    // block at most one needs a quotient, so the ways are told apart by predicates, ONE division runs on the selected operands and the
    // result is routed by selects: no divergent branches (the nested form cost ~200 instructions per cloudy level, this one ~70).
    const bool act = !last, up = cn >= cl;
    const double fmx = fmax(cl, cp), fmn = fmin(cl, cp);
    const bool u_f = act && up && first && cl < 1.;                 // facclr2 = (cn - cl) / (1 - cl)
    const bool u_gt = act && up && !first && cn > fmx;              // facclr1 = rat2, facclr2 = (cn - fmx) / (1 - fmx)
    const bool u_lt = act && up && !first && cn < fmx;              // facclr1 = (cn - cl) / (cp - cl)
    const bool u_eq = act && up && !first && !(cn > fmx) && !(cn < fmx);      // facclr1 = rat2
    const bool d_f = act && !up && first;                           // faccld2 = (cl - cn) / cl
    const bool d_le = act && !up && !first && cn <= fmn;            // faccld1 = rat1, faccld2 = (fmn - cn) / fmn
    const bool d_gt = act && !up && !first && !(cn <= fmn);         // faccld1 = (cl - cn) / (cl - fmn)
    double num = 0.0, den = 1.0;
    num = u_f ? cn - cl : num;     den = u_f ? 1. - cl : den;
    num = u_gt ? cn - fmx : num;   den = u_gt ? 1. - fmx : den;
    num = u_lt ? cn - cl : num;    den = u_lt ? cp - cl : den;
    num = d_f ? cl - cn : num;     den = d_f ? cl : den;
    num = d_le ? fmn - cn : num;   den = d_le ? fmn : den;
    num = d_gt ? cl - cn : num;    den = d_gt ? cl - fmn : den;
    const double q = fdiv(num, den);
    const double clr1 = (u_gt || u_eq) ? rat2 : (u_lt ? q : 0.0);
    const double clr2 = (u_f || u_gt) ? q : 0.0;
    const double cld1 = d_le ? rat1 : (d_gt ? q : 0.0);
    const double cld2 = (d_f || d_le) ? q : 0.0;
    const bool r1 = (act && up) ? (clr1 > 0. || clr2 > 0.) : (act ? false : brat1);
    const bool r2 = (act && !up) ? (cld1 > 0. || cld2 > 0.) : (act ? false : brat2);
    double cmb1 = 0.0, cmb2 = 0.0;
    if (!first) {
        const double cx = last ? 0.0 : cn;          // beyond the last level the reference's neighbour fraction is taken as 0
        cmb1 = fmax(0., fmin(cx - cl, cp - cl));
        cmb2 = fmax(0., fmin(cl - cx, cl - cp));
    }
    return OvlFac{clr1, cld1, cmb1, cmb2, clr2, cld2, r1, r2};
}

// cflag[lay][col]: bit 0 = the layer holds cloud for the sweeps (cldfrac >= 1e-6), bits 8.. = cldprop's ncbands in effect at the layer;
// cflag[0][col] bit 3 = the column holds cloud.  mode 2 (rtrnmr): the overlap factors of every cloudy level for both sweep directions
// (the reference's two set-up loops, rtrnmr :347-506) go to W.ovl, "first cloudy level of a block" to bits 1 (downward) and 2 (upward).
template <bool GCM>
__global__ __launch_bounds__(256) void k_cloudscan(Workspace W, GcmIn g, ColIn c, int ncol, int col0, int nct, int inflag, int iceflag, int liqflag, int mode)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    const int nlay = W.nlay;
    int top = 0, bot = nlay + 1;
    if (col < ncol) {
    const size_t gc = (size_t)col0 + pcol(W, col);
    const double *cldfr = GCM ? g.cldfr : c.cldfrac;
    const double *ciwp_ = GCM ? g.cicewp : c.ciwp, *clwp_ = GCM ? g.cliqwp : c.clwp;
    int ncbands = 1, anycloud = 0;
    const size_t ncb = W.ncolb;
    bool prevcld = false, rat1 = false, rat2 = false;       // upward sweep order = this loop's order
    double cfprev = 0.0;
#pragma unroll 4
    for (int lay = 1; lay <= nlay; lay++) {
        const size_t gi = gc + (size_t)nct * (lay - 1);
        const double cf = cldfr[gi], ciwp = ciwp_[gi], clwp = clwp_[gi];
        const double cwp = ciwp + clwp;
        bool enters = cf >= 1.e-20 && cwp >= 1.e-20;
        if (cf >= 1.e-20 && !enters) enters = cloud_layer_enters(cf, cwp, cloud_tauctot<GCM>(g, c, gc, gi, nct, lay));
        if (enters) {
            if (inflag == 0 || inflag == 1) ncbands = 16;
            else if (inflag == 2) {
                if (ciwp != 0.0) { if (iceflag == 1) ncbands = 5; else if (iceflag == 2 || iceflag == 3) ncbands = 16; }
                if (clwp != 0.0 && liqflag == 1) ncbands = 16;
            }
        }
        const int cloudy = cf >= 1.e-6;
        if (cloudy && !anycloud) bot = lay;
        anycloud |= cloudy;
        if (cloudy) top = lay;
        int first = 0;
        if (mode == 2) {
            if (cloudy) {
                first = !prevcld;
                const OvlFac mf = mr_step(cf, lay < nlay ? cldfr[gi + nct] : 0.0, cfprev, first, lay == nlay, rat1, rat2);
                rat1 = mf.rat1; rat2 = mf.rat2;
                prevcld = true;
                cfprev = cf;
                double2 *o = W.ovl + ((size_t)((nlay + 1) + lay) * 3) * ncb + col;
                o[0] = make_double2(mf.clr1, mf.cld1); o[ncb] = make_double2(mf.cmb1, mf.cmb2); o[2 * ncb] = make_double2(mf.clr2, mf.cld2);
            } else prevcld = false;
        }
        W.cflag[(size_t)lay * ncb + col] = cloudy | (first << 2) | (ncbands << 8);
    }
    if (mode == 2 && anycloud) {            // downward sweep order
        prevcld = false; rat1 = false; rat2 = false; cfprev = 0.0;
        for (int lay = top; lay >= 1; lay--) {
            const size_t gi = gc + (size_t)nct * (lay - 1);
            const double cf = cldfr[gi];
            if (cf >= 1.e-6) {
                const bool first = !prevcld;
                const OvlFac mf = mr_step(cf, lay > 1 ? cldfr[gi - nct] : 0.0, cfprev, first, lay == 1, rat1, rat2);
                rat1 = mf.rat1; rat2 = mf.rat2;
                prevcld = true;
                cfprev = cf;
                double2 *o = W.ovl + ((size_t)lay * 3) * ncb + col;
                o[0] = make_double2(mf.clr1, mf.cld1); o[ncb] = make_double2(mf.cmb1, mf.cmb2); o[2 * ncb] = make_double2(mf.clr2, mf.cld2);
                if (first) W.cflag[(size_t)lay * ncb + col] |= 2;
            } else prevcld = false;
        }
    }
    W.ncbands[col] = ncbands;
    W.cflag[col] = anycloud ? 8 : 0;
    W.cflag[(size_t)(nlay + 1) * W.ncolb + col] = 0;
    }
    // highest and lowest cloudy layer of the block: the 64 columns of a block are one workgroup (one wave) of this kernel (a cloud-free
    // column holds 0 / nlay + 1); written, not raised with atomics: nothing has to initialise them in front of this kernel
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { top = max(top, __shfl_xor(top, o, 64)); bot = min(bot, __shfl_xor(bot, o, 64)); }
    if (threadIdx.x == 0 && col < ncol) { W.btop[col >> 6] = top; W.bbot[col >> 6] = bot; }
}

// k_cloudlay : cldprop for one (column, layer) (src/rrtmg_lw_cldprop.f90:173-293) and the cloud optical depth along the diffusivity
//              angle per SPECTRAL band (rtrn :321-349 / rtrnmr :333-343).  mode 1 = rtrn (also the effective emissivity term), 2 = rtrnmr.
template <bool GCM>
__global__ __launch_bounds__(256) void k_cloudlay(DevTables T, Workspace W, GcmIn g, ColIn c, int ncol, int col0, int nct, int mode,
                                                  int inflag, int iceflag, int liqflag)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncol) return;
    const int lay = blockIdx.y + 1;
    const size_t gc = (size_t)col0 + pcol(W, col);
    const int nlay = W.nlay;
    const size_t ncb = W.ncolb;
    const size_t gi = gc + (size_t)nct * (lay - 1);
    const double *S = T.stat;
    const double *absice1 = S + T.sl.absice1, *absice2 = S + T.sl.absice2, *absice3 = S + T.sl.absice3, *absliq1 = S + T.sl.absliq1;
    const double cf = (GCM ? g.cldfr : c.cldfrac)[gi];
    const double ciwp = (GCM ? g.cicewp : c.ciwp)[gi], clwp = (GCM ? g.cliqwp : c.clwp)[gi];
    const int flagword = W.cflag[(size_t)lay * ncb + col];
    const int cloudy = flagword & 1, nb_at = flagword >> 8;       // the band count cldprop had reached when it worked on this layer
    const int ncbands = W.ncbands[col];                            // ... and at the end of the column: rtrn's band -> cloud-band map (:343-349)
    const double cwp = ciwp + clwp;
    bool enters = cf >= 1.e-20 && cwp >= 1.e-20;
    if (cf >= 1.e-20 && !enters) enters = cloud_layer_enters(cf, cwp, cloud_tauctot<GCM>(g, c, gc, gi, nct, lay));
    // inflag 2: how the ice / liquid absorption coefficients of this layer are evaluated (cldprop :199-262)
    int err = 0, icemode = -1, liqmode = -1, iceind = 0, liqind = 0, index_i = 1, index_l = 1;
    double radice = 0.0, ice_single = 0.0, fint_i = 0.0, liq_single = 0.0, fint_l = 0.0;
    if (enters && inflag == 2) {
        radice = (GCM ? g.reice : c.rei)[gi];
        if (ciwp == 0.0) { icemode = 0; ice_single = 0.0; iceind = 0; }
        else if (iceflag == 0) {
            if (radice < 10.0) err = E_ICE_SMALL;
            icemode = 0; ice_single = T.absice0[0] + T.absice0[1] / radice; iceind = 0;
        } else if (iceflag == 1) {
            if (radice < 13.0 || radice > 130.) err = E_ICE_BOUNDS;
            icemode = 1; iceind = 1;
        } else if (iceflag == 2) {
            if (radice < 5.0 || radice > 131.0) err = E_ICE_BOUNDS;
            const double factor = (radice - 2.) / 3.;
            index_i = (int)factor; if (index_i == 43) index_i = 42;
            fint_i = factor - (double)index_i;
            icemode = 2; iceind = 2;
        } else if (iceflag == 3) {
            if (radice < 5.0 || radice > 140.0) err = E_ICE_GEN_BOUNDS;
            const double factor = (radice - 2.) / 3.;
            index_i = (int)factor; if (index_i == 46) index_i = 45;
            fint_i = factor - (double)index_i;
            icemode = 3; iceind = 2;
        } else err = E_BAD_FLAG;
        if (clwp == 0.0) { liqmode = 0; liq_single = 0.0; liqind = 0; if (iceind == 1) iceind = 2; }
        else if (liqflag == 0) { liqmode = 0; liq_single = T.absliq0; liqind = 0; if (iceind == 1) iceind = 2; }
        else if (liqflag == 1) {
            const double radliq = (GCM ? g.reliq : c.rel)[gi];
            if ((radliq < 2.5 || radliq > 60.) && !err) err = E_LIQ_BOUNDS;      // (both sizes out: the reference stops at the ice check, :212-244)
            index_l = (int)(radliq - 1.5);
            if (index_l == 0) index_l = 1;
            if (index_l == 58) index_l = 57;
            fint_l = radliq - 1.5 - (double)index_l;
            liqmode = 1; liqind = 2;
        } else err = E_BAD_FLAG;
        if (err) index_i = clampi(index_i, 1, 42), index_l = clampi(index_l, 1, 57);
    }
    if (err) atomicCAS(W.err, 0, err);
    if (!cloudy) return;          // k_layer and the sweeps read odcld / efcl of cloudy layers only
    // cloud bands of the final count, each written to the spectral bands it serves
    for (int ib = 1; ib <= ncbands; ib++) {
        double t = 0.0;                                             // taucloud(lay, ib)
        if (enters && ib <= nb_at) {
            if (inflag == 0) t = GCM ? g.taucld[(ib - 1) + (size_t)NBND * gi] : c.tauc[gc + (size_t)nct * ((ib - 1) + (size_t)NBND * (lay - 1))];
            else if (inflag == 1) t = T.abscld1 * cwp;
            else if (inflag == 2) {
                int ki = icb_map(ib, iceind);
                const int kl = icb_map(ib, liqind);
                // iceflag = 1 (Ebert-Curry) has five ice bands.  When another layer of the column made cldprop carry 16 bands (liqflag = 1
                // with liquid water) and this layer is ice only, the reference promotes iceind to 2 and reads abscoice(6:16), values left over
                // from an earlier layer or call (src/rrtmg_lw_cldprop.f90:215-222,252-258,283-286: ill-defined upstream).  Bands 1-5 are the
                // reference's; bands 6-16 of such a layer use the fifth Ebert-Curry band here instead of reading past the 5 x 2 table.
                if (icemode == 1 && ki > 5) ki = 5;
                double ai, al;
                if (icemode == 0) ai = ice_single;
                else if (icemode == 1) ai = absice1[2 * (ki - 1)] + absice1[2 * (ki - 1) + 1] / radice;
                else if (icemode == 2) { const double *tb = absice2 + 43 * (ki - 1); ai = tb[index_i - 1] + fint_i * (tb[index_i] - tb[index_i - 1]); }
                else if (icemode == 3) { const double *tb = absice3 + 46 * (ki - 1); ai = tb[index_i - 1] + fint_i * (tb[index_i] - tb[index_i - 1]); }
                else ai = 0.0;
                if (liqmode == 0) al = liq_single;
                else if (liqmode == 1) { const double *tb = absliq1 + 58 * (kl - 1); al = tb[index_l - 1] + fint_l * (tb[index_l] - tb[index_l - 1]); }
                else al = 0.0;
                t = ciwp * ai + clwp * al;
            }
        }
        // optical depth along the diffusivity angle; secdiff is indexed by the CLOUD band ib (rtrn :323)
        const double od = W.percol[(size_t)(PC_SECDIFF + ib - 1) * ncb + col] * t;
        double ef = 0.0;
        if (mode == 1) ef = (1. - exp(-od)) * cf;
        // spectral bands served by cloud band ib: rtrn :343-349
        int Blo = ib, Bhi = ib;
        if (ncbands == 1) { Blo = 1; Bhi = NBND; }
        else if (ncbands == 5) { Blo = ib <= 2 ? ib : (ib == 3 ? 3 : (ib == 4 ? 6 : 9)); Bhi = ib <= 2 ? ib : (ib == 3 ? 5 : (ib == 4 ? 8 : NBND)); }
        for (int B = Blo; B <= Bhi; B++) {
            const size_t o = ((size_t)(B - 1) * nlay + (lay - 1)) * ncb + col;
            W.odcld[o] = od;
            if (mode == 1) W.efcl[o] = ef;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_blocksort : orders the 64-column blocks of a batch by their highest cloudy layer, deepest first (a counting sort, equal tops in
//               block order: the result does not depend on timing), pads the order to whole groups of SORT_GROUP with the block number
//               "one past the last" (columns past the end: every sweep lane of such a block is masked), and gives every group the
//               top of its first = deepest block as hand-off level.  The reference decides clear / cloudy per (column, layer)
//               (icldlyr, src/rrtmg_lw_rtrnmr.f90:509-704); this is that decision at the granularity of a wavefront's 64 columns:
//               above a block's hand-off level the total-sky stream IS the clear-sky stream.  One workgroup; nblk <= SORT_MAXBLK.
// ------------------------------------------------------------------------------------------------
constexpr int SORT_GROUP = 12;                  // divisible by every column-block count of a sweep workgroup (nsb_fit)
constexpr int SORT_MAXBLK = 16384;              // 1 048 576 columns per batch
constexpr int SORT_MAXLAY = 603;                // parrrtm.f90:31 mxlay
__host__ __device__ constexpr int nsb_fit(int n) { return n >= 12 ? 12 : n >= 6 ? 6 : n >= 4 ? 4 : n >= 3 ? 3 : n >= 2 ? 2 : 1; }
__host__ __device__ constexpr int sort_slots(int nblk) { return (nblk + SORT_GROUP - 1) / SORT_GROUP * SORT_GROUP; }

__global__ __launch_bounds__(256) void k_blocksort(Workspace W, int nblk, int force_top)
{
    __shared__ unsigned short s_top[SORT_MAXBLK];
    __shared__ int s_cnt[SORT_MAXLAY + 1], s_start[SORT_MAXLAY + 1], s_gtop[SORT_MAXBLK / SORT_GROUP + 1];
    const int tid = threadIdx.x, nth = blockDim.x, nlay = W.nlay, nslot = sort_slots(nblk), ngrp = nslot / SORT_GROUP;
    for (int v = tid; v <= nlay; v += nth) s_cnt[v] = 0;
    __syncthreads();
    for (int b = tid; b < nblk; b += nth) {
        const int t = min(max(W.btop[b], 0), nlay);
        s_top[b] = (unsigned short)t;
        atomicAdd(&s_cnt[t], 1);
    }
    __syncthreads();
    // first position of every value, deepest first: an exclusive prefix sum over u = nlay - v by the first wave (each lane a run of values)
    if (tid < 64) {
        const int per = (nlay + 64) / 64, u0 = tid * per;
        int sum = 0;
        for (int u = u0; u < u0 + per && u <= nlay; u++) sum += s_cnt[nlay - u];
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (tid >= o) incl += t; }
        int pos = incl - sum;
        for (int u = u0; u < u0 + per && u <= nlay; u++) { s_start[nlay - u] = pos; pos += s_cnt[nlay - u]; }
    }
    __syncthreads();
    // top of the first block of every group: the value whose run [start, start + count) holds position SORT_GROUP g (the starts grow with
    // u = nlay - v: binary search for the last u with start <= q; runs of count 0 share their start with the next non-empty one, which the
    // search passes over because it looks for the LAST such u ... of a non-empty run: step back over empty ones)
    for (int g = tid; g < ngrp; g += nth) {
        const int q = SORT_GROUP * g;           // (< nblk: the last group starts below nblk)
        int lo = 0, hi = nlay;                  // largest u with s_start[nlay - u] <= q
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_start[nlay - mid] <= q) lo = mid; else hi = mid - 1; }
        while (lo > 0 && s_cnt[nlay - lo] == 0) lo--;      // (an empty run at the end of equal starts)
        // force_top (a batch too small to fill the chip): every group hands off at the top of the column, i.e. the cloud-zone sweep walks
        // all levels - with its clear-sky body below the lowest cloud and its clear-sky branch above the highest - and the two clear-sky
        // launches, each a latency chain of its own, are not made (driver.hip: one_sweep).  Same numbers: a level's partial does not depend
        // on the kernel that swept it.
        const int top = force_top ? nlay : nlay - lo;
        s_gtop[g] = top;
        W.hgrp[g] = top;
    }
    __syncthreads();
    // placement by the first wave, 64 blocks at a time in block order: the lanes that hold the same value as the first unplaced lane take
    // consecutive positions of that value's run (a handful of distinct values per 64 blocks)
    if (tid < 64) {
        for (int b0 = 0; b0 < nblk; b0 += 64) {
            const int b = b0 + tid;
            const bool in = b < nblk;
            const int v = in ? (int)s_top[b] : -1;
            unsigned long long todo = __builtin_amdgcn_ballot_w64(in);
            while (todo) {
                const int lead = __builtin_ctzll(todo);
                const int lv = __shfl(v, lead, 64);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(in && v == lv) & todo;
                const int base = s_start[lv];
                if (in && v == lv) {
                    const int p = base + __builtin_popcountll(m & ((1ull << tid) - 1ull));
                    W.order[p] = b;
                    W.hblk[b] = s_gtop[p / SORT_GROUP];
                }
                __builtin_amdgcn_wave_barrier();
                if (tid == lead) s_start[lv] = base + __builtin_popcountll(m);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                todo &= ~m;
            }
        }
    }
    for (int p = nblk + tid; p < nslot; p += nth) W.order[p] = nblk;
    __syncthreads();                    // (the order written by the first wave is read below)
    // lowest cloudy layer of every group (a group without cloud: nlay + 1; its hand-off level is 0 and nothing is swept in the zone)
    for (int g = tid; g < ngrp; g += nth) {
        int b = nlay + 1;
        for (int p = SORT_GROUP * g; p < SORT_GROUP * (g + 1) && p < nblk; p++) b = min(b, W.bbot[W.order[p]]);
        W.hbot[g] = b;
    }
}

// ------------------------------------------------------------------------------------------------
// Band descriptions for taumol (src/rrtmg_lw_taumol.f90:299-3164; compact spec: SURVEY.md appendix B)
// ------------------------------------------------------------------------------------------------
enum Sp { H2O = 0, CO2, O3, N2O, CO, CH4, O2, BRD };                 // F_COLH2O + Sp
enum Key { K_NONE, K_SINGLE, K_BINARY, K_ZERO };
enum Amt { A_COL, A_ADJ, A_BRD_N2, A_O2, A_BRD };
enum Rat { R_H2OCO2 = 0, R_H2OO3, R_H2ON2O, R_H2OCH4, R_N2OCO2, R_O3CO2 };
enum Corr { C_NONE, C_B1LO, C_B1UP, C_B2LO };

struct Minor {
    Amt amt; int sp; bool two_d; int refslot;
    double thr, base, expo;    // A_ADJ parameters
    double chiconst;           // > 0: literal reference mixing ratio (band 13); else chi_mls(sp, jp+1)
};
struct Region {
    Key key; int a, b, rat;
    bool self_, for_;
    int planck_slot;           // >= 0: Planck fractions interpolated in the mixture (refrat slot); -1: constant
    bool frac_from_a;          // upper region takes its (constant) fractions from fracrefa (band 6)
    int nm; Minor m[3];
    int ncfc; int cfc_wx[2];
    Corr corr;
    int mult;                  // 0 none, 4 = band-4 upper multipliers, 7 = band-7 upper multipliers
};
constexpr Minor NOM = {A_COL, 0, false, 0, 0, 0, 0, 0};
constexpr Region ZERO_REGION = {K_ZERO, 0, 0, 0, false, false, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0};

template <int B> struct BT;
#ifdef RRLW_G256
#define BAND_NG(NG_) 16
#else
#define BAND_NG(NG_) NG_
#endif
#define BAND_TRAITS(B_, NG_, LO, UP) \
    template <> struct BT<B_> { static constexpr int ng = BAND_NG(NG_); static constexpr Region lo = LO; static constexpr Region up = UP; };

#define R1(...) Region{__VA_ARGS__}
BAND_TRAITS(1, 10,
    R1(K_SINGLE, H2O, 0, 0, true, true, -1, false, 1, {{A_BRD_N2, BRD, false, 0, 0, 0, 0, 0}, NOM, NOM}, 0, {0, 0}, C_B1LO, 0),
    R1(K_SINGLE, H2O, 0, 0, false, true, -1, false, 1, {{A_BRD_N2, BRD, false, 0, 0, 0, 0, 0}, NOM, NOM}, 0, {0, 0}, C_B1UP, 0))
BAND_TRAITS(2, 12,
    R1(K_SINGLE, H2O, 0, 0, true, true, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_B2LO, 0),
    R1(K_SINGLE, H2O, 0, 0, false, true, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
BAND_TRAITS(3, 16,
    R1(K_BINARY, H2O, CO2, R_H2OCO2, true, true, 0, false, 1, {{A_ADJ, N2O, true, 2, 1.5, 0.5, 0.65, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_BINARY, H2O, CO2, R_H2OCO2, false, true, 1, false, 1, {{A_ADJ, N2O, true, 3, 1.5, 0.5, 0.65, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
BAND_TRAITS(4, 14,
    R1(K_BINARY, H2O, CO2, R_H2OCO2, true, true, 0, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_BINARY, O3, CO2, R_O3CO2, false, false, 1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 4))
BAND_TRAITS(5, 16,
    R1(K_BINARY, H2O, CO2, R_H2OCO2, true, true, 0, false, 1, {{A_COL, O3, true, 2, 0, 0, 0, 0}, NOM, NOM}, 1, {1, 0}, C_NONE, 0),
    R1(K_BINARY, O3, CO2, R_O3CO2, false, false, 1, false, 0, {NOM, NOM, NOM}, 1, {1, 0}, C_NONE, 0))
BAND_TRAITS(6, 8,
    R1(K_SINGLE, H2O, 0, 0, true, true, -1, false, 1, {{A_ADJ, CO2, false, 0, 3.0, 2.0, 0.77, 0}, NOM, NOM}, 2, {2, 3}, C_NONE, 0),
    R1(K_NONE, 0, 0, 0, false, false, -1, true, 0, {NOM, NOM, NOM}, 2, {2, 3}, C_NONE, 0))
BAND_TRAITS(7, 12,
    R1(K_BINARY, H2O, O3, R_H2OO3, true, true, 0, false, 1, {{A_ADJ, CO2, true, 2, 3.0, 3.0, 0.79, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_SINGLE, O3, 0, 0, false, false, -1, false, 1, {{A_ADJ, CO2, false, 0, 3.0, 2.0, 0.79, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 7))
BAND_TRAITS(8, 8,
    R1(K_SINGLE, H2O, 0, 0, true, true, -1, false, 3,
       {{A_ADJ, CO2, false, 0, 3.0, 2.0, 0.65, 0}, {A_COL, O3, false, 0, 0, 0, 0, 0}, {A_COL, N2O, false, 0, 0, 0, 0, 0}}, 2, {3, 4}, C_NONE, 0),
    R1(K_SINGLE, O3, 0, 0, false, false, -1, false, 2,
       {{A_ADJ, CO2, false, 0, 3.0, 2.0, 0.65, 0}, {A_COL, N2O, false, 0, 0, 0, 0, 0}, NOM}, 2, {3, 4}, C_NONE, 0))
BAND_TRAITS(9, 12,
    R1(K_BINARY, H2O, CH4, R_H2OCH4, true, true, 0, false, 1, {{A_ADJ, N2O, true, 2, 1.5, 0.5, 0.65, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_SINGLE, CH4, 0, 0, false, false, -1, false, 1, {{A_ADJ, N2O, false, 0, 1.5, 0.5, 0.65, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
BAND_TRAITS(10, 6,
    R1(K_SINGLE, H2O, 0, 0, true, true, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_SINGLE, H2O, 0, 0, false, true, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
BAND_TRAITS(11, 8,
    R1(K_SINGLE, H2O, 0, 0, true, true, -1, false, 1, {{A_O2, O2, false, 0, 0, 0, 0, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_SINGLE, H2O, 0, 0, false, true, -1, false, 1, {{A_O2, O2, false, 0, 0, 0, 0, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
BAND_TRAITS(12, 8,
    R1(K_BINARY, H2O, CO2, R_H2OCO2, true, true, 0, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    ZERO_REGION)
BAND_TRAITS(13, 4,
    R1(K_BINARY, H2O, N2O, R_H2ON2O, true, true, 0, false, 2,
       {{A_ADJ, CO2, true, 2, 3.0, 2.0, 0.68, 3.55e-4}, {A_COL, CO, true, 4, 0, 0, 0, 0}, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_NONE, 0, 0, 0, false, false, -1, false, 1, {{A_COL, O3, false, 0, 0, 0, 0, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
BAND_TRAITS(14, 2,
    R1(K_SINGLE, CO2, 0, 0, true, true, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_SINGLE, CO2, 0, 0, false, false, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
BAND_TRAITS(15, 2,
    R1(K_BINARY, N2O, CO2, R_N2OCO2, true, true, 0, false, 1, {{A_BRD, BRD, true, 2, 0, 0, 0, 0}, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    ZERO_REGION)
BAND_TRAITS(16, 2,
    R1(K_BINARY, H2O, CH4, R_H2OCH4, true, true, 0, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0),
    R1(K_SINGLE, CH4, 0, 0, false, false, -1, false, 0, {NOM, NOM, NOM}, 0, {0, 0}, C_NONE, 0))
#undef R1

__device__ const double kMult4[16] = {1, 1, 1, 1, 1, 1, 1, 0.92, 0.88, 1.07, 1.1, 0.99, 0.88, 0.943, 1, 1};   // taumol :1028-1034
__device__ const double kMult7[16] = {1, 1, 1, 1, 1, 0.92, 0.88, 1.07, 1.1, 0.99, 0.855, 1, 1, 1, 1, 1};      // taumol :1664-1669 (g 6-11 of the band, whatever its size)

// setcoef results of one (layer, column), kept in registers by k_layer
struct LayerCoef {
    double f[NFIELD];
    int jp, jt, jt1, indself, indfor, indminor;
};

struct Spec { double speccomb, specparm, fs; int js; };
__device__ __forceinline__ Spec spec_calc(double cola, double rat, double colb, double mult, double oneminus)
{
    Spec s;                                         // taumol :523-528
    s.speccomb = cola + rat * colb;
    s.specparm = fdiv(cola, s.speccomb);
    if (s.specparm >= oneminus) s.specparm = oneminus;
    const double specmult = mult * s.specparm;
    s.js = 1 + (int)specmult;
    s.fs = specmult - (double)(int)specmult;        // mod(specmult, 1.0) for specmult >= 0
    return s;
}

// lower-atmosphere binary stencil, branch-free form of taumol :569-598 / :641-663:
// rows ind+off+{0,1,2} and ind+off+9+{0,1,2} with weights w[0..5] (unused points get weight 0)
__device__ __forceinline__ void stencil6(double specparm, double fs, double fa, double fb, int &off, double (&w)[6])
{
    if (specparm < 0.125) {
        const double p = fs - 1, p2 = p * p, p4 = p2 * p2;
        const double fk0 = p4, fk1 = 1 - p - 2.0 * p4, fk2 = p + p4;
        off = 0;
        w[0] = fk0 * fa; w[1] = fk1 * fa; w[2] = fk2 * fa; w[3] = fk0 * fb; w[4] = fk1 * fb; w[5] = fk2 * fb;
    } else if (specparm > 0.875) {
        const double p = -fs, p2 = p * p, p4 = p2 * p2;
        const double fk0 = p4, fk1 = 1 - p - 2.0 * p4, fk2 = p + p4;
        off = -1;
        w[0] = fk2 * fa; w[1] = fk1 * fa; w[2] = fk0 * fa; w[3] = fk2 * fb; w[4] = fk1 * fb; w[5] = fk0 * fb;
    } else {
        off = 0;
        w[0] = (1. - fs) * fa; w[1] = fs * fa; w[2] = 0.0; w[3] = (1. - fs) * fb; w[4] = fs * fb; w[5] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// taumol as a sparse linear combination.  For one (layer, column) and band, the gaseous optical depth of
// every g-point is   tau(g) = sum_i  w_i * K[off_i + g]   over a handful of table rows: the P/T(/mixture)
// interpolation stencil of the key species, the two self- and two foreign-continuum rows, 2 or 4 rows per
// minor gas, one row per halocarbon (src/rrtmg_lw_taumol.f90:299-3164).  rows_prep
// turns the layer's setcoef quantities into the (off_i, w_i) list once; rows_eval then needs only the g-offset.
// The weights are algebraically those of the reference (e.g. selffac*(1-selffrac), selffac*selffrac for
// selffac*(s0 + selffrac*(s1-s0))); products are associated differently, i.e. results differ at rounding level.
// ------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int region_nrows(const Region &R, bool lower)
{
    int n = 0;
    if (R.key == K_SINGLE) n += 4;
    else if (R.key == K_BINARY) n += lower ? 12 : 8;
    if (R.self_) n += 2;
    if (R.for_) n += 2;
    for (int i = 0; i < R.nm; i++) n += R.m[i].two_d ? 4 : 2;
    n += R.ncfc;
    return n;
}

__host__ __device__ constexpr int region_major_rows(const Region &R, bool lower)
{
    return R.key == K_SINGLE ? 4 : (R.key == K_BINARY ? (lower ? 12 : 8) : 0);
}
__host__ __device__ constexpr int region_minor_base(const Region &R, bool lower, int im)
{
    int n = region_major_rows(R, lower) + (R.self_ ? 2 : 0) + (R.for_ ? 2 : 0);
    for (int i = 0; i < im; i++) n += R.m[i].two_d ? 4 : 2;
    return n;
}

// g-point "quads": every band is padded to a multiple of 4 g-points; quad q of the 38 holds g-points
// QG0(band) + 4*(q - QSTART(band)) ... +3 of one band.  Scratch arrays are [array][quad][layer][column][4].
#ifdef RRLW_G256
__host__ __device__ constexpr int band_ng(int B) { return B >= 1 ? 16 : 16; }
#else
__host__ __device__ constexpr int band_ng(int B) { return B == 1 ? 10 : B == 2 ? 12 : B == 3 ? 16 : B == 4 ? 14 : B == 5 ? 16 : B == 6 ? 8 : B == 7 ? 12 :
                                                    B == 8 ? 8 : B == 9 ? 12 : B == 10 ? 6 : B == 11 ? 8 : B == 12 ? 8 : B == 13 ? 4 : 2; }
#endif
__host__ __device__ constexpr int band_nquad(int B) { return (band_ng(B) + 3) / 4; }
__host__ __device__ constexpr int band_qstart(int B)     // not recursive: a recursive constexpr function that is not folded becomes a
{                                                       // real device call with a dynamic stack
    int s = 0;
    for (int b = 1; b < B; b++) s += band_nquad(b);
    return s;
}
constexpr int NQUAD = band_qstart(17);      // 38
__host__ __device__ constexpr int band_g0(int B)      // 0-based first g-point of band B among the 140
{
    int s = 0;
    for (int b = 1; b < B; b++) s += band_ng(b);
    return s;
}
static_assert(band_g0(17) == NGPT, "g-point table");
static_assert(NQUAD == (NGPT == 140 ? 38 : 64), "quad table");

// setcoef's chi_mls ratios and mixing ratios (6 x 59 and 7 x 59 doubles, contiguous in the static buffer): rows_prep reads two or three
// of them per band and needs them at once; k_layer copies them into LDS once per workgroup (a global read costs ~500 cycles of
// exposed latency each, 16 bands x 3).
constexpr int NRATCHI = 6 * 59 + 7 * 59;
__shared__ double s_ratchi[NRATCHI];

template <int N>
struct Rows {
    unsigned off[N > 0 ? N : 1];   // element offsets into the packed k-table buffer (row start, g = 0)
    double w[N > 0 ? N : 1];
    unsigned fw;                   // binary-key regions: Planck fractions are interpolated between rows js-1 and js of fracrefa/b with
                                   // weight fs (taumol :556-561, :692-693); packed (js << 28) | fs in 28-bit fixed point for the sweeps
};

// binary-key bands get a slot in Workspace::fw (every band whose upper region is binary-key has a binary-key lower region too)
template <int B> constexpr unsigned lo_binary_mask() { return (BT<B>::lo.key == K_BINARY ? 1u << (B - 1) : 0u) | lo_binary_mask<B - 1>(); }
template <> constexpr unsigned lo_binary_mask<0>() { return 0u; }
template <int B> constexpr unsigned up_binary_mask() { return (BT<B>::up.key == K_BINARY ? 1u << (B - 1) : 0u) | up_binary_mask<B - 1>(); }
template <> constexpr unsigned up_binary_mask<0>() { return 0u; }
template <int B> constexpr unsigned up_zero_mask() { return (BT<B>::up.key == K_ZERO ? 1u << (B - 1) : 0u) | up_zero_mask<B - 1>(); }
template <> constexpr unsigned up_zero_mask<0>() { return 0u; }
template <int B> constexpr unsigned up_from_a_mask() { return (BT<B>::up.frac_from_a ? 1u << (B - 1) : 0u) | up_from_a_mask<B - 1>(); }
template <> constexpr unsigned up_from_a_mask<0>() { return 0u; }
constexpr unsigned LO_BINARY = lo_binary_mask<16>(), UP_BINARY = up_binary_mask<16>(), UP_ZERO = up_zero_mask<16>(), UP_FROM_A = up_from_a_mask<16>();
static_assert((UP_BINARY & ~LO_BINARY) == 0u, "fw slots are assigned by the lower region");
__host__ __device__ constexpr int popcnt_c(unsigned v) { int n = 0; for (; v; v &= v - 1) n++; return n; }
constexpr int NFW = popcnt_c(LO_BINARY);                                          // 9
__host__ __device__ constexpr int fw_slot(int B) { return popcnt_c(LO_BINARY & ((1u << (B - 1)) - 1u)); }

// one minor gas: rows IBASE.. of the list
template <int B, bool LOWER, int N, int IM>
__device__ __forceinline__ void rows_prep_minor(const DevTables &T, const LayerCoef &C, Rows<N> &rw)
{
    constexpr Region R = LOWER ? BT<B>::lo : BT<B>::up;
    constexpr unsigned ng = BT<B>::ng;
    constexpr Minor M = R.m[IM];
    constexpr int I0 = region_minor_base(R, LOWER, IM);
    const BandLayout &L = T.band[B - 1];
    const double mf = C.f[F_MINORFRAC];
    double amount;
    if constexpr (M.amt == A_COL) amount = C.f[F_COLH2O + M.sp];
    else if constexpr (M.amt == A_BRD_N2) amount = C.f[F_COLBRD] * C.f[F_SCALEMINORN2];
    else if constexpr (M.amt == A_O2) amount = C.f[F_COLO2] * C.f[F_SCALEMINOR];
    else if constexpr (M.amt == A_BRD) amount = C.f[F_COLBRD] * C.f[F_SCALEMINOR];
    else {                                              // A_ADJ: taumol :547-554
        const double colx = C.f[F_COLH2O + M.sp], coldry = C.f[F_COLDRY];
        const double chiref = M.chiconst > 0. ? M.chiconst : s_ratchi[(T.sl.chi - T.sl.rat) + M.sp * 59 + C.jp];     // chi_mls(sp+1, jp+1)
        const double chi = fdiv(colx, coldry);
        const double ratx = fdiv(1.e20 * chi, chiref);
        amount = colx;
        if (ratx > M.thr) amount = (M.base + pow(ratx - M.base, M.expo)) * chiref * coldry * 1.e-20;
    }
    const unsigned slot = (unsigned)(LOWER ? L.minor_lo[IM] : L.minor_up[IM]);
    if constexpr (M.two_d) {                            // taumol :635-639
        constexpr unsigned nj = LOWER ? 9 : 5;
        const Spec sm = spec_calc(C.f[F_COLH2O + R.a], T.refrat[B - 1][M.refslot], C.f[F_COLH2O + R.b], LOWER ? 8. : 4., T.oneminus);
        const unsigned r = slot + ((unsigned)(C.indminor - 1) * nj + (unsigned)(sm.js - 1)) * ng;
        rw.off[I0] = r;                    rw.w[I0] = amount * ((1. - mf) * (1. - sm.fs));
        rw.off[I0 + 1] = r + ng;           rw.w[I0 + 1] = amount * ((1. - mf) * sm.fs);
        rw.off[I0 + 2] = r + nj * ng;      rw.w[I0 + 2] = amount * (mf * (1. - sm.fs));
        rw.off[I0 + 3] = r + nj * ng + ng; rw.w[I0 + 3] = amount * (mf * sm.fs);
    } else {
        const unsigned r = slot + (unsigned)(C.indminor - 1) * ng;
        rw.off[I0] = r;          rw.w[I0] = amount * (1. - mf);
        rw.off[I0 + 1] = r + ng; rw.w[I0 + 1] = amount * mf;
    }
}

template <int B, bool LOWER, int N>
__device__ __forceinline__ void rows_prep(const DevTables &T, const LayerCoef &C, Rows<N> &rw)
{
    constexpr Region R = LOWER ? BT<B>::lo : BT<B>::up;
    constexpr unsigned ng = BT<B>::ng;
    const BandLayout &L = T.band[B - 1];
    const int jp = C.jp, jt = C.jt, jt1 = C.jt1;
    const double *rat_tab = s_ratchi;
    rw.fw = 0u;
    if constexpr (R.key == K_ZERO) return;

    double corradj = 1.;
    if constexpr (R.corr == C_B1LO) { if (C.f[F_PAVEL] < 250.) corradj = 1. - 0.15 * (250. - C.f[F_PAVEL]) / 154.4; }
    else if constexpr (R.corr == C_B1UP) corradj = 1. - 0.15 * (C.f[F_PAVEL] / 95.6);
    else if constexpr (R.corr == C_B2LO) corradj = 1. - .05 * (C.f[F_PAVEL] - 100.) / 900.;

    if constexpr (R.key == K_SINGLE) {                      // taumol :356-360
        const unsigned r0 = LOWER ? ((jp - 1) * 5 + (jt - 1)) : ((jp - 13) * 5 + (jt - 1));
        const unsigned r1 = LOWER ? (jp * 5 + (jt1 - 1)) : ((jp - 12) * 5 + (jt1 - 1));
        const unsigned tab = (unsigned)(LOWER ? L.absa : L.absb);
        const double colk = C.f[F_COLH2O + R.a];
        rw.off[0] = tab + r0 * ng;       rw.w[0] = colk * C.f[F_FAC00];
        rw.off[1] = tab + (r0 + 1) * ng; rw.w[1] = colk * C.f[F_FAC10];
        rw.off[2] = tab + r1 * ng;       rw.w[2] = colk * C.f[F_FAC01];
        rw.off[3] = tab + (r1 + 1) * ng; rw.w[3] = colk * C.f[F_FAC11];
    } else if constexpr (R.key == K_BINARY) {
        const double cola = C.f[F_COLH2O + R.a], colb = C.f[F_COLH2O + R.b];
        const double rat = rat_tab[R.rat * 59 + (jp - 1)], rat_1 = rat_tab[R.rat * 59 + jp];
        constexpr double mult = LOWER ? 8. : 4.;
        const Spec s = spec_calc(cola, rat, colb, mult, T.oneminus);
        const Spec s1 = spec_calc(cola, rat_1, colb, mult, T.oneminus);
        if constexpr (LOWER) {                              // taumol :563-663
            const unsigned tab = (unsigned)L.absa;
            const int ind0 = ((jp - 1) * 5 + (jt - 1)) * 9 + s.js - 1;      // 0-based row
            const int ind1 = (jp * 5 + (jt1 - 1)) * 9 + s1.js - 1;
            int so;
            double w6[6];
            stencil6(s.specparm, s.fs, C.f[F_FAC00], C.f[F_FAC10], so, w6);
            unsigned r = tab + (unsigned)(ind0 + so) * ng;
            rw.off[0] = r;           rw.w[0] = s.speccomb * w6[0];
            rw.off[1] = r + ng;      rw.w[1] = s.speccomb * w6[1];
            rw.off[2] = r + 2 * ng;  rw.w[2] = s.speccomb * w6[2];
            rw.off[3] = r + 9 * ng;  rw.w[3] = s.speccomb * w6[3];
            rw.off[4] = r + 10 * ng; rw.w[4] = s.speccomb * w6[4];
            rw.off[5] = r + 11 * ng; rw.w[5] = s.speccomb * w6[5];
            stencil6(s1.specparm, s1.fs, C.f[F_FAC01], C.f[F_FAC11], so, w6);
            r = tab + (unsigned)(ind1 + so) * ng;
            rw.off[6] = r;            rw.w[6] = s1.speccomb * w6[0];
            rw.off[7] = r + ng;       rw.w[7] = s1.speccomb * w6[1];
            rw.off[8] = r + 2 * ng;   rw.w[8] = s1.speccomb * w6[2];
            rw.off[9] = r + 9 * ng;   rw.w[9] = s1.speccomb * w6[3];
            rw.off[10] = r + 10 * ng; rw.w[10] = s1.speccomb * w6[4];
            rw.off[11] = r + 11 * ng; rw.w[11] = s1.speccomb * w6[5];
        } else {                                            // taumol :749-771
            const unsigned tab = (unsigned)L.absb;
            const unsigned ind0 = ((jp - 13) * 5 + (jt - 1)) * 5 + s.js - 1;
            const unsigned ind1 = ((jp - 12) * 5 + (jt1 - 1)) * 5 + s1.js - 1;
            unsigned r = tab + ind0 * ng;
            rw.off[0] = r;          rw.w[0] = s.speccomb * ((1. - s.fs) * C.f[F_FAC00]);
            rw.off[1] = r + ng;     rw.w[1] = s.speccomb * (s.fs * C.f[F_FAC00]);
            rw.off[2] = r + 5 * ng; rw.w[2] = s.speccomb * ((1. - s.fs) * C.f[F_FAC10]);
            rw.off[3] = r + 6 * ng; rw.w[3] = s.speccomb * (s.fs * C.f[F_FAC10]);
            r = tab + ind1 * ng;
            rw.off[4] = r;          rw.w[4] = s1.speccomb * ((1. - s1.fs) * C.f[F_FAC01]);
            rw.off[5] = r + ng;     rw.w[5] = s1.speccomb * (s1.fs * C.f[F_FAC01]);
            rw.off[6] = r + 5 * ng; rw.w[6] = s1.speccomb * ((1. - s1.fs) * C.f[F_FAC11]);
            rw.off[7] = r + 6 * ng; rw.w[7] = s1.speccomb * (s1.fs * C.f[F_FAC11]);
        }
        // Planck fractions interpolated in the mixture: taumol :556-561, :692-693
        const Spec sp = spec_calc(cola, T.refrat[B - 1][R.planck_slot], colb, mult, T.oneminus);
        unsigned q = (unsigned)(sp.fs * 268435456.0 + 0.5);
        if (q > 268435455u) q = 268435455u;
        rw.fw = ((unsigned)sp.js << 28) | q;
    }
    constexpr int IS = region_major_rows(R, LOWER);
    if constexpr (R.self_) {                                // taumol :350-351
        const unsigned r = (unsigned)L.selfref + (unsigned)(C.indself - 1) * ng;
        rw.off[IS] = r;          rw.w[IS] = C.f[F_SELFFAC] * (1. - C.f[F_SELFFRAC]);
        rw.off[IS + 1] = r + ng; rw.w[IS + 1] = C.f[F_SELFFAC] * C.f[F_SELFFRAC];
    }
    constexpr int IF = IS + (R.self_ ? 2 : 0);
    if constexpr (R.for_) {                                 // taumol :352-353
        const unsigned r = (unsigned)L.forref + (unsigned)(C.indfor - 1) * ng;
        rw.off[IF] = r;          rw.w[IF] = C.f[F_FORFAC] * (1. - C.f[F_FORFRAC]);
        rw.off[IF + 1] = r + ng; rw.w[IF + 1] = C.f[F_FORFAC] * C.f[F_FORFRAC];
    }
    if constexpr (R.nm > 0) rows_prep_minor<B, LOWER, N, 0>(T, C, rw);
    if constexpr (R.nm > 1) rows_prep_minor<B, LOWER, N, 1>(T, C, rw);
    if constexpr (R.nm > 2) rows_prep_minor<B, LOWER, N, 2>(T, C, rw);
    constexpr int IC = region_minor_base(R, LOWER, R.nm);   // halocarbons: taumol :1254, :1381-1382, :1753-1754
    if constexpr (R.ncfc > 0) { rw.off[IC] = (unsigned)L.vec[0]; rw.w[IC] = C.f[F_WX1 + R.cfc_wx[0] - 1]; }
    if constexpr (R.ncfc > 1) { rw.off[IC + 1] = (unsigned)L.vec[1]; rw.w[IC + 1] = C.f[F_WX1 + R.cfc_wx[1] - 1]; }
    static_assert(IC + R.ncfc == N, "row count");
    if constexpr (R.corr != C_NONE) {
#pragma unroll
        for (int i = 0; i < N; i++) rw.w[i] = corradj * rw.w[i];
    }
}

// 16-byte table load through a buffer descriptor: 32-bit per-lane byte offset, no 64-bit address arithmetic,
// and the hardware range check returns zeros for anything outside the table buffer.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double2 ld2(__amdgpu_buffer_rsrc_t rsrc, unsigned elem_off)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(elem_off * 8u), 0, 0);
    double2 d;
    __builtin_memcpy(&d, &v, 16);
    return d;
}

// the same 16 bytes from the band's tables staged in LDS (element offset into the staging buffer)
__device__ __forceinline__ double2 ldl(const double2 *lds, unsigned elem_off) { return lds[elem_off >> 1]; }

// Workgroup barrier that orders LDS accesses only.  __syncthreads() is a workgroup-scope release / acquire over ALL address spaces: on
// gfx950 that puts `s_waitcnt vmcnt(0)` in front of the barrier, and k_layer's waves then sit out the acknowledgement of every code
// store of the band they have just finished (stores count in vmcnt) sixteen times per layer although no other wave reads those codes.
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// In-kernel stamps (diagnostic build -DRRLW_LAYER_STAMPS only: where a k_layer wave spends its cycles; the build's run time means
// nothing, its SHARES do).  Segment sums per wave in LDS, added to g_stamps at the end of the kernel; rrtmg_lw_hip_debug_stamps reads them.
#ifdef RRLW_LAYER_STAMPS
constexpr int NSTAMP = 8;
__device__ unsigned long long g_stamps[NSTAMP + 1];
__shared__ unsigned long long s_stamp[16 * (NSTAMP + 1)];
__device__ __forceinline__ void stamp(int seg)
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *w = s_stamp + (threadIdx.x >> 6) * (NSTAMP + 1);
        if (seg >= 0) w[seg] += t - w[NSTAMP];
        w[NSTAMP] = t;
    }
}
#define STAMP(seg) stamp(seg)
#else
#define STAMP(seg) ((void)0)
#endif

// ------------------------------------------------------------------------------------------------
// Staging of the bands' tables in LDS.  The table evaluation returns ~15 KB of table rows per (layer, column) to registers; through the
// vector L1 that is bound by its 64 B/clk return path (measured: 90 % of it), LDS returns 256 B/clk.  All threads of a k_layer
// workgroup work on the SAME layer, so they need the same few pressure planes of the key-species tables and the same few temperature
// slices of the minor-gas tables: the workgroup stages, per band, the planes jp0 .. jp0+2 (jp0 = its smallest reference-pressure index;
// a cell uses planes jp and jp+1), MINOR_WIN slices of each minor-gas table from im0 = its smallest minor-gas temperature index (a
// cell uses slices indminor and indminor+1), the whole self / foreign / halocarbon tables, and evaluates from LDS.  A wave with a cell
// outside the window (other region of the atmosphere, jp > jp0 + 1, indminor > im0 + MINOR_WIN - 2) evaluates from global memory -
// same values either way.
// Bands are staged in PASSES of several bands (LayerPasses, below): in-kernel stamps (tools/stamps_run.py) showed a wave spending 30 %
// of its cycles between the barriers of the sixteen per-band staging rounds and 7 % at the barrier in front of each; a pass is ONE
// round - the tables of up to eleven bands, as one flat list of 16-byte pieces - and the windowed minor-gas tables make four passes
// of the sixteen bands.
// ------------------------------------------------------------------------------------------------
enum Role { RL_MAJOR, RL_SELF, RL_FOR, RL_MINOR0, RL_MINOR1, RL_MINOR2, RL_CFC0, RL_CFC1, NROLE };

#ifndef RRLW_MINOR_WIN
#define RRLW_MINOR_WIN 6          // temperature slices (7.2 K each) of a minor-gas table staged per workgroup; 19 = the whole table
#endif
constexpr int MINOR_WIN = RRLW_MINOR_WIN;
static_assert(MINOR_WIN >= 2 && MINOR_WIN <= 19, "minor-gas tables have 19 temperature slices");
// The staging window of a workgroup comes in two sizes (round 5, profiles/round5_orography.md).  NARROW - three pressure planes (cells
// with jp0 <= jp <= jp0 + 1), MINOR_WIN minor-gas slices - where the 256 columns of the layer lie that close together: a pressure grid
// that is (nearly) the same in every column.  WIDE - five planes (jp0 .. jp0 + 3), ten slices, the bands in more passes - where they do
// not: a terrain-following grid puts the columns of one model level at surface-pressure factors of 0.55 .. 1.03 (three reference planes
// apart, setcoef :276-284) and at temperatures 30 K apart.  Chosen per workgroup from the spread of its cells; with the narrow window
// alone half of such a grid's waves fell to the global-memory evaluation and k_layer took 37.7 ms instead of 23 per 1e6 columns.
template <int NPL_, int MW_> struct StageWin { static constexpr int NPL = NPL_, MW = MW_; };
using WinNarrow = StageWin<3, MINOR_WIN>;
#ifdef RRLW_G256
using WinWide = WinNarrow;               // (the 256-g-point build keeps the narrow window: its tables are twice the size)
constexpr bool HAVE_WIDE = false;
#else
using WinWide = StageWin<5, 10>;
constexpr bool HAVE_WIDE = true;
#endif

template <int B, bool LOWER, class WN>
struct Stage {
    static constexpr Region R = LOWER ? BT<B>::lo : BT<B>::up;
    static constexpr int ng = BT<B>::ng;
    static constexpr int nsp = R.key == K_BINARY ? (LOWER ? 9 : 5) : 1;          // mixture points per (P, T) node
    static constexpr int NPL = WN::NPL;                                          // pressure planes staged
    static constexpr bool has_major = R.key == K_SINGLE || R.key == K_BINARY;
    static constexpr int major_rows = has_major ? NPL * 5 * nsp + 3 : 0;         // + 3: zero-weight stencil rows may lie past the last plane
    static constexpr int nj(int k) { return R.m[k].two_d ? (LOWER ? 9 : 5) : 1; }   // rows per temperature slice of minor gas k
    static constexpr int mrows(int k) { return k < R.nm ? WN::MW * nj(k) : 0; }
    // doubles of the segment with role `r`, and its start within the band's part of the staging buffer (segments follow each other)
    static constexpr int n(int r)
    {
        return r == RL_MAJOR ? major_rows * ng : r == RL_SELF ? (R.self_ ? 10 * ng : 0) : r == RL_FOR ? (R.for_ ? 4 * ng : 0) :
               r == RL_MINOR0 ? mrows(0) * ng : r == RL_MINOR1 ? mrows(1) * ng : r == RL_MINOR2 ? mrows(2) * ng :
               r == RL_CFC0 ? (R.ncfc > 0 ? ng : 0) : (R.ncfc > 1 ? ng : 0);
    }
    static constexpr int l(int r) { int s = 0; for (int q = 0; q < r; q++) s += n(q); return s; }
    static constexpr int total = l(NROLE);
};

#ifndef RRLW_LAYER_BLOCK
#define RRLW_LAYER_BLOCK 256      // (measured: 192 threads 29.9 ms, 256 25.5, 384 43.0, 512 35.5 per 1e6 cloudy columns)
#endif
constexpr int LAYER_BLOCK = RRLW_LAYER_BLOCK;   // threads of a k_layer workgroup: three workgroups per CU (a 47 KB staging buffer each), three waves per SIMD
#ifndef RRLW_STAGE_DOUBLES
#define RRLW_STAGE_DOUBLES 5800   // capacity of the staging buffer: three workgroups per CU, each 46 400 B + 6 136 B of chi / ratio tables + flags = 52 552 B (the LDS is handed out in pieces of 2 KB: 53 248 x 3 of the 163 840 B)
#endif
constexpr int STAGE_DOUBLES = RRLW_STAGE_DOUBLES;

// the bands of one staging pass, in evaluation order
template <int... Bs> struct BandList { static constexpr int b[sizeof...(Bs)] = {Bs...}; static constexpr int n = sizeof...(Bs); };
// start of band number I of the pass within the staging buffer, in doubles
template <class PL, bool LOWER, class WN, int I> constexpr int pass_base()
{
    if constexpr (I == 0) return 0;
    else return pass_base<PL, LOWER, WN, I - 1>() + Stage<PL::b[I - 1], LOWER, WN>::total;
}
template <class PL, bool LOWER, class WN> constexpr int pass_total() { return pass_base<PL, LOWER, WN, PL::n>(); }

// where each segment of band B comes from: element offsets into the packed table buffer (wave-uniform: scalar registers)
template <int B, bool LOWER, class WN>
__device__ __forceinline__ void stage_sources(const DevTables &T, int jp0, int im0, unsigned (&g)[NROLE])
{
    using S = Stage<B, LOWER, WN>;
    constexpr Region R = S::R;
    constexpr int ng = S::ng;
    const BandLayout &L = T.band[B - 1];
#pragma unroll
    for (int r = 0; r < NROLE; r++) g[r] = 0u;
    if constexpr (S::has_major) {
        const int plane0 = LOWER ? jp0 - 1 : jp0 - 13;
        g[RL_MAJOR] = (unsigned)(LOWER ? L.absa : L.absb) + (unsigned)(plane0 * 5 * S::nsp * ng);
    }
    if constexpr (R.self_) g[RL_SELF] = (unsigned)L.selfref;
    if constexpr (R.for_) g[RL_FOR] = (unsigned)L.forref;
    if constexpr (R.nm > 0) g[RL_MINOR0] = (unsigned)(LOWER ? L.minor_lo[0] : L.minor_up[0]) + (unsigned)((im0 - 1) * S::nj(0) * ng);
    if constexpr (R.nm > 1) g[RL_MINOR1] = (unsigned)(LOWER ? L.minor_lo[1] : L.minor_up[1]) + (unsigned)((im0 - 1) * S::nj(1) * ng);
    if constexpr (R.nm > 2) g[RL_MINOR2] = (unsigned)L.minor_lo[2] + (unsigned)((im0 - 1) * S::nj(2) * ng);
    if constexpr (R.ncfc > 0) g[RL_CFC0] = (unsigned)L.vec[0];
    if constexpr (R.ncfc > 1) g[RL_CFC1] = (unsigned)L.vec[1];
}

// The staging buffer of a pass is the bands' segments one after the other; a thread copies the 16-byte pieces tid, tid + 256, ...
// Per-lane source offsets of those pieces: of the segments, whose bounds are compile-time constants, only the few that meet the 256
// pieces of round k contribute a compare and a select.
template <class PL, bool LOWER, class WN, int I, int IT>
__device__ __forceinline__ void pass_offsets(const DevTables &T, int jp0, int im0, int tid, unsigned (&off)[IT])
{
    if constexpr (I < PL::n) {
        using S = Stage<PL::b[I], LOWER, WN>;
        constexpr int base = pass_base<PL, LOWER, WN, I>();
        unsigned g[NROLE];
        stage_sources<PL::b[I], LOWER, WN>(T, jp0, im0, g);
#pragma unroll
        for (int r = 0; r < NROLE; r++) {
            const int n = S::n(r), lo = (base + S::l(r)) / 2, hi = lo + n / 2;         // constants once the loops are unrolled
            if (n > 0) {
#pragma unroll
                for (int k = 0; k < IT; k++) {
                    if (hi > LAYER_BLOCK * k && lo < LAYER_BLOCK * (k + 1)) {
                        const int c = tid + LAYER_BLOCK * k;
                        const unsigned src = g[r] + 2u * (unsigned)(c - lo);
                        off[k] = (lo <= LAYER_BLOCK * k || c >= lo) ? src : off[k];
                    }
                }
            }
        }
        pass_offsets<PL, LOWER, WN, I + 1, IT>(T, jp0, im0, tid, off);
    }
}

// two-phase copy: every thread first issues ALL its 16-byte loads (at most 12, independent), then writes them to LDS - a pass costs one
// memory round trip
template <class PL, bool LOWER, class WN>
__device__ __forceinline__ void stage_pass(const DevTables &T, __amdgpu_buffer_rsrc_t kt, double2 *lds, int jp0, int im0, int tid)
{
    constexpr int NCH = pass_total<PL, LOWER, WN>() / 2;
    constexpr int IT = (NCH + LAYER_BLOCK - 1) / LAYER_BLOCK;
    static_assert(pass_total<PL, LOWER, WN>() <= STAGE_DOUBLES, "the pass does not fit the staging buffer");
    if constexpr (IT > 0) {
        unsigned off[IT];
#pragma unroll
        for (int k = 0; k < IT; k++) off[k] = 0u;
        pass_offsets<PL, LOWER, WN, 0, IT>(T, jp0, im0, tid, off);
        double2 v[IT];
#pragma unroll
        for (int k = 0; k < IT; k++) v[k] = ld2(kt, off[k]);          // (past the last piece: some table data or, past the buffer, zeros; not stored)
#pragma unroll
        for (int k = 0; k < IT; k++) {
            const int c = tid + LAYER_BLOCK * k;
            if (c < NCH) lds[c] = v[k];
        }
    }
}

// packed-table offset -> staging-buffer offset, per role, for band B whose part of the buffer starts at BASE
template <int B, bool LOWER, class WN, int BASE>
__device__ __forceinline__ void band_delta(const DevTables &T, int jp0, int im0, unsigned (&delta)[NROLE])
{
    unsigned g[NROLE];
    stage_sources<B, LOWER, WN>(T, jp0, im0, g);
#pragma unroll
    for (int r = 0; r < NROLE; r++) delta[r] = (unsigned)(BASE + Stage<B, LOWER, WN>::l(r)) - g[r];
}

// row offsets of the packed table buffer -> offsets into the staging buffer (rows_prep's row order: key species, self, foreign, minors, halocarbons)
template <int B, bool LOWER, int N>
__device__ __forceinline__ void rows_to_lds(Rows<N> &rw, const unsigned (&delta)[NROLE])
{
    constexpr Region R = LOWER ? BT<B>::lo : BT<B>::up;
    constexpr int IS = region_major_rows(R, LOWER), IF = IS + (R.self_ ? 2 : 0), IM0 = IF + (R.for_ ? 2 : 0);
    constexpr int IM1 = region_minor_base(R, LOWER, 1), IM2 = region_minor_base(R, LOWER, 2), IC = region_minor_base(R, LOWER, R.nm);
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int role = i < IS ? RL_MAJOR : i < IF ? RL_SELF : i < IM0 ? RL_FOR :
                         (i < IC ? (R.nm > 1 && i >= IM1 ? (R.nm > 2 && i >= IM2 ? RL_MINOR2 : RL_MINOR1) : RL_MINOR0) : (i == IC ? RL_CFC0 : RL_CFC1));
        rw.off[i] = rw.off[i] + delta[role];
    }
}

// Optical depth of ALL g-points of band B (padded to whole quads with zeros).  The table loads of a band are all independent, so
// they are issued as a software pipeline: the band's loads form one list (row-major: N rows x ng/2 16-byte loads), cut into chunks
// of RRLW_LOAD_CHUNK; chunk c+1 is in flight while chunk c is consumed.  sched_barrier keeps the compiler from hoisting every load
// to the top (which spills) or sinking them to their uses (which serialises the latency again).  LDS = the rows come from the
// workgroup's staging buffer (rw.off then holds staging offsets, rows_to_lds), otherwise from global memory through the vector L1.
#ifndef RRLW_LOAD_CHUNK
#define RRLW_LOAD_CHUNK 2       // loads in flight per pipeline stage.  From LDS two suffice (8 were needed through the vector L1) and the
#endif                          // registers saved allow three waves per SIMD: 36.4 vs 40.9 ms per 1e6 cloudy columns

template <int B, bool LOWER, int N>
struct BandLoads {
    static constexpr Region R = LOWER ? BT<B>::lo : BT<B>::up;
    static constexpr int ng = BT<B>::ng;
    static constexpr int HP = ng / 2;                                    // 16-byte loads per table row
    static constexpr int NK = N * HP;                                    // absorption-coefficient loads
    static constexpr int NL = NK;
    static constexpr int CH = RRLW_LOAD_CHUNK;
    static constexpr int NCH = (NL + CH - 1) / CH;

    template <int C, bool LDS>
    static __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t kt, const double2 *lds, const Rows<N> &rw, double2 (&b)[CH])
    {
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const int idx = C * CH + k;
            if (idx < NK) b[k] = LDS ? ldl(lds, rw.off[idx / HP] + 2u * (unsigned)(idx % HP)) : ld2(kt, rw.off[idx / HP] + 2u * (unsigned)(idx % HP));
        }
    }

    template <int C>
    static __device__ __forceinline__ void consume(const Rows<N> &rw, const double2 (&b)[CH], double *tau)
    {
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const int idx = C * CH + k;
            if (idx < NK) {
                const int i = idx / HP, p = idx % HP;
                tau[2 * p] = tau[2 * p] + rw.w[i] * b[k].x;
                tau[2 * p + 1] = tau[2 * p + 1] + rw.w[i] * b[k].y;
            }
        }
    }

    template <int C, bool LDS>
    static __device__ __forceinline__ void step(__amdgpu_buffer_rsrc_t kt, const double2 *lds, const Rows<N> &rw, double2 (&cur)[CH], double2 (&nxt)[CH],
                                                double *tau)
    {
        if constexpr (C < NCH) {
            if constexpr (C + 1 < NCH) issue<C + 1, LDS>(kt, lds, rw, nxt);
            __builtin_amdgcn_sched_barrier(0);
            consume<C>(rw, cur, tau);
            __builtin_amdgcn_sched_barrier(0);
            step<C + 1, LDS>(kt, lds, rw, nxt, cur, tau);
        }
    }
};

// tau0: what the sum starts from - the layer's aerosol optical depth of the band (taut = taug + taua, src/rrtmg_lw_rad.nomcica.f90:527-539),
// so that the sum arrives complete (one addition per cell less; with taua = 0, the usual case, bit for bit what it was).  The two regions
// whose gas optical depth is scaled per g-point afterwards (bands 4 and 7 above the tropopause) start from 0 and add taua behind the factor.
template <int B, bool LOWER, int N, bool LDS>
__device__ __forceinline__ void rows_eval_band(__amdgpu_buffer_rsrc_t kt, const double2 *lds, const Rows<N> &rw, double tau0, double (&tau)[4 * band_nquad(B)])
{
    using BL = BandLoads<B, LOWER, N>;
    constexpr int NP = 4 * band_nquad(B);
    constexpr bool SCALED = BL::R.mult != 0;
#pragma unroll
    for (int j = 0; j < NP; j++) tau[j] = (SCALED || j >= BL::ng) ? 0.0 : tau0;
    if constexpr (BL::NL > 0) {
        double2 b0[BL::CH], b1[BL::CH];
        BL::template issue<0, LDS>(kt, lds, rw, b0);
        BL::template step<0, LDS>(kt, lds, rw, b0, b1, tau);
    }
    if constexpr (SCALED) {
#pragma unroll
        for (int j = 0; j < BL::ng; j++) {
            if constexpr (BL::R.mult == 4) tau[j] = fma(tau[j], kMult4[j], tau0);
            else if constexpr (BL::R.mult == 7) tau[j] = fma(tau[j], kMult7[j], tau0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_layer : for one (column, layer):  inatm's layer part (src/rrtmg_lw_rad.nomcica.f90:785-867), setcoef
//           (src/rrtmg_lw_setcoef.f90:276-429), taumol for all bands (src/rrtmg_lw_taumol.f90:299-3164), taut = taug +
//           taua (src/rrtmg_lw_rad.nomcica.f90:527-539) and, per g-point, the optical depth along the diffusivity angle and
//           the branch rtrn's sweep body takes on it (src/rrtmg_lw_rtrn.f90:362-451) as a 4-byte code (cell_code).
//           Results go to the [quad][layer][column][4] code arrays.
// ------------------------------------------------------------------------------------------------
struct LayerArgs {
    int ncol, col0, nct, idrv, istart, iend;
    // a batch that does not fill the chip: the bands of a (window, layer) over `nparts` workgroups (grid.z, or grid.y of the wide launch),
    // workgroup p takes the bands of partmask[p] (bit B - 1); 0 / 1: one workgroup takes them all
    int nparts;
    unsigned partmask[4];
    int ktab_bytes;            // size of the packed k-table buffer (buffer descriptor range)
    const double *tauaer;      // (nct,nlay,16)
};

struct alignas(16) scr4 { scr_t v[4]; };

// The per-cell codes are written once by k_layer and read twice (down and up sweep) by k_sweepc / k_sweepz, gigabytes later: streaming
// (non-temporal) stores here and loads there (bload_scr4_nt) keep them from evicting the absorption tables from L2.
typedef float scr_vec __attribute__((ext_vector_type(4)));
// a quad's four codes as they lie in memory
struct pk4 { unsigned w[CODE_WORDS]; };
__device__ __forceinline__ pk4 pack4(const scr4 &v)
{
    pk4 p;
#pragma unroll
    for (int k = 0; k < 4; k++) p.w[k] = __float_as_uint(v.v[k]);
    return p;
}
__device__ __forceinline__ scr4 unpack4(const pk4 &p)
{
    scr4 v;
#pragma unroll
    for (int k = 0; k < 4; k++) v.v[k] = __uint_as_float(p.w[k]);
    return v;
}
typedef unsigned pk_vec __attribute__((ext_vector_type(CODE_WORDS)));
// (Round 5 measured this store against a cached one, +0.3 ... +1.7 ms, and against two knock-outs with wrong results - codes formed and
// not stored 17.6 ms, half of every record stored 20.3: profiles/round5_instruction_diet.md.)
__device__ __forceinline__ void scr_store(unsigned *base, size_t cell, const scr4 &v)
{
    const pk4 p = pack4(v);
    pk_vec x;
#pragma unroll
    for (int k = 0; k < CODE_WORDS; k++) x[k] = p.w[k];
    __builtin_nontemporal_store(x, reinterpret_cast<pk_vec *>(base + cell * CODE_WORDS));
}
// transmittance-table index of an optical depth: rtrn :445 (tblint = 10000, Pade constant bpade)
__device__ __forceinline__ int lut_index(double od, double bpade) { return (int)(10000.0 * fdiv(od, bpade + od) + 0.5); }

// code of a series-branch cell: its optical depth as a float, negative values (and NaN) to zero - the clamp modifier of the conversion
// ([0, 1]; a thin cell is <= 0.06)
__device__ __forceinline__ scr_t thin_code(double od) { return __builtin_amdgcn_fmed3f((scr_t)od, 0.0f, 1.0f); }

// table indices of the four cells of a quad, formed together when any of them is thick (see gas_codes); a thin cell's index is not used
__device__ __forceinline__ void quad_indices(double o0, double o1, double o2, double o3, bool t0, bool t1, bool t2, bool t3, double bpade, int *ig)
{
    ig[0] = ig[1] = ig[2] = ig[3] = 0;
    if (t0 || t1 || t2 || t3) {
        ig[0] = lut_index(o0, bpade); ig[1] = lut_index(o1, bpade); ig[2] = lut_index(o2, bpade); ig[3] = lut_index(o3, bpade);
    }
}
__device__ __forceinline__ void quad_indices(double o0, double o1, double o2, double o3, double bpade, int *ig)
{
    quad_indices(o0, o1, o2, o3, !(o0 <= 0.06), !(o1 <= 0.06), !(o2 <= 0.06), !(o3 <= 0.06), bpade, ig);
}

// What k_layer hands to the sweeps for one cell is the DECISION the reference takes on its optical depth (rtrn :372-451), in 4 bytes:
//   code >= 0 : the optical depth itself (<= 0.06, or odtot < 0.06) - the series branch: atrans = od - od^2/2, tfac = od/6
//   code <  0 : -(index into the 1e-4-quantised transmittance / tfn tables), formed here in float64 exactly as the reference forms it
// The sweep turns the code back into (transmittance, tfn factor) and forms the Planck source terms in float64 itself.  Compared with
// storing {atrans, bbd, bbu} as three floats this is a third of the bytes, and the table index never depends on a rounded value.
__device__ __forceinline__ scr_t cell_code(double od, bool series, double bpade)
{
    return series ? (scr_t)od : -(scr_t)lut_index(od, bpade);
}

// all cells (g-points) of band B of one (layer, column).
// CLOUD: 0 clear-sky set, 1 one cloud optical depth per band (rtrn / rtrnmr), 2 one per g-point from W.odg (rtrnmc, sub-column
// arrays), 3 the band's value where the sub-column mask has a bit (rtrnmc, generator mask; gbits = the band's ng mask bits)
// 5 (CL_SHARE): 3, and the cells' optical depths - secdiff x (gas + aerosol), as they stand in front of the codes - are stored as
// float64 in W.odg: the first sample of a call that averages several sub-column samples (rrtmg_lw_hip_run_mcica_samples).  They do not
// depend on the sample; k_codet forms the total codes of the later samples from them, and k_layer does not run again.
constexpr int CL_SHARE = 5;
template <int B, int CLOUD, bool LOWER, int N, bool LDS>
__device__ __forceinline__ void band_cells(const DevTables &T, const Workspace &W, __amdgpu_buffer_rsrc_t kt, const double2 *lds, const Rows<N> &rw, int lay, int col,
                                           bool incol, double secdiff, double taua, int cloudy, double odcld, unsigned gbits)
{
    constexpr Region R = LOWER ? BT<B>::lo : BT<B>::up;
    constexpr int ng = BT<B>::ng;
    constexpr int NQ = band_nquad(B), NP = 4 * NQ, QS = band_qstart(B);
    const int nlay = W.nlay;
    const size_t ncb = W.ncolb;
    double od[NP];
    rows_eval_band<B, LOWER, N, LDS>(kt, lds, rw, taua, od);
    const double *S = T.stat;
    const double *__restrict__ tau_tbl = S + T.sl.tau_tbl;
    const double bpade = T.bpade;
    // (kept in the basic block of the table loads: an instruction-sinking pass would otherwise move the whole FMA chains
    // below the next branch and keep every loaded row alive until then)
#pragma unroll
    for (int j = 0; j < NP; j++) {        // optical depth along the diffusivity angle: rtrn :368-369
        // The reference's `if (odepth < 0) odepth = 0` is NOT applied here: a negative value is a thin cell, and its code is formed with
        // the conversion's clamp modifier (thin_code: one instruction, where a float64 compare and two selects per cell stood until round
        // 5; fmax(o, 0) - one v_max_f64 - makes the scheduler overlap more of the band and spills 29 registers: this kernel sits at its
        // 168-register budget).  The cloudy branch, which adds the cloud optical depth to this value, clamps it first (below).
        double o = secdiff * od[j];          // (od: gas + aerosol, rows_eval_band)
        if (j >= ng) o = 0.0;
        od[j] = o;
    }
#pragma unroll
    for (int j = 0; j < NP; j++) asm volatile("" : "+v"(od[j]));   // pin: the values exist here (LLVM's Sink pass may not move their FMA chains past this point)
    STAMP(3);
    // (the stores stay inside `if (incol)`: made unconditional - lanes past the last column write what the last column writes - the
    // scheduler moves code across them and spills 26 registers: 24.4 -> 31.5 ms)
    if constexpr (R.key == K_BINARY) { if (incol) W.fw[((size_t)fw_slot(B) * nlay + (lay - 1)) * ncb + col] = rw.fw; }
    const size_t so0 = ((size_t)QS * nlay + (lay - 1)) * ncb + col;     // scratch cell of the band's first quad
    const size_t qstride = (size_t)nlay * ncb;
    if constexpr (CLOUD == CL_SHARE) {
        if (incol) {
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                double2 *po = reinterpret_cast<double2 *>(W.odg + (so0 + q * qstride) * 4);
                po[0] = double2{od[4 * q], od[4 * q + 1]};
                po[1] = double2{od[4 * q + 2], od[4 * q + 3]};
            }
        }
    }
    // gas: series for od <= 0.06, else the table (rtrn :372-451; in a cloudy layer the branch taken for the gas terms depends on od alone)
    auto gas_codes = [&]() {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            scr4 c;
            // the table index costs a float64 division (~14 instructions per cell, a third of k_layer's arithmetic): formed for the four
            // cells of a QUAD together when any of them is thick (the g-points of a band are ordered by absorption: thick cells are
            // neighbours) and skipped for a wave whose quad is all thin (upper atmosphere, band wings).  One exec-mask bracket per quad
            // instead of one per cell - a quarter of the scalar instructions - and four independent division chains in flight instead
            // of one after the other (round 5: profiles/round5_instruction_diet.md).
            const bool t0 = !(od[4 * q] <= 0.06), t1 = !(od[4 * q + 1] <= 0.06), t2 = !(od[4 * q + 2] <= 0.06), t3 = !(od[4 * q + 3] <= 0.06);
#pragma unroll
            for (int k = 0; k < 4; k++) c.v[k] = thin_code(od[4 * q + k]);
            if (t0 || t1 || t2 || t3) {
                const scr_t i0 = -(scr_t)lut_index(od[4 * q], bpade), i1 = -(scr_t)lut_index(od[4 * q + 1], bpade);
                const scr_t i2 = -(scr_t)lut_index(od[4 * q + 2], bpade), i3 = -(scr_t)lut_index(od[4 * q + 3], bpade);
                c.v[0] = t0 ? i0 : c.v[0]; c.v[1] = t1 ? i1 : c.v[1]; c.v[2] = t2 ? i2 : c.v[2]; c.v[3] = t3 ? i3 : c.v[3];
            }
            if (incol) scr_store(W.scr[S_CODE], so0 + q * qstride, c);
            __builtin_amdgcn_sched_barrier(0);      // (one quad's chains at a time: all of a band's at once cost registers this kernel does not have)
        }
    };
    if constexpr (CLOUD == 0) {
        gas_codes();
    } else {
        // A wave with a cloudy lane (all 64 columns sit in the same layer) forms, per group of quads, the table index of the thick cells ONCE
        // and uses it for the gas code and for the cloudy branch p3 (round 3: the two passes of round 2 divided twice; a cloudy layer cost
        // 3.2 x a clear one).  The three sub-branches of rtrn :372-435:
        //   p1: odtot < 0.06              total from the series
        //   p2: else if odepth <= 0.06    total = odepth + odcld from the table
        //   p3: else                      odepth := tau_tbl(itgas), total from the table
        // (McICA, CLOUD 2 / 3: every g-point has its own cloud optical depth - eight more live doubles per quad in flight; with two quads
        // the kernel spilled 13-18 registers)
        // (the per-g-point flavours keep the two passes: with the index held across the group they spilled 7-9 registers)
        constexpr bool REUSE = CLOUD == 1;
        const bool wave_cloudy = __builtin_amdgcn_ballot_w64(cloudy != 0) != 0ull;
        if (!REUSE || !wave_cloudy) gas_codes();
        if (wave_cloudy) {
#pragma unroll
            for (int j = 0; j < ng; j++) { if (!(od[j] >= 0.0)) od[j] = 0.0; }       // rtrn :369 (see above)
            // QC: quads of a band whose cloudy-layer look-ups are in flight together (2 until round 5: with the quad-wise table indices
            // two spill ten registers - profiles/round5_instruction_diet.md).  The loops over the QC quads of a group stay although QC is
            // 1: written out for one quad the kernel compiles to other code (162 registers instead of 168, 3.6 KB more of it), which
            // a change that is to leave the code object alone cannot take (profiles/switch_retirement.md).
            constexpr int QC = 1;
#pragma unroll
            for (int q0 = 0; q0 < NQ; q0 += QC) {
                constexpr int GC = 4 * QC;
                int ig[REUSE ? GC : 1];     // table index of the gas optical depth, 0 for a series cell
                if constexpr (REUSE) {
#pragma unroll
                    for (int q = 0; q < QC; q++) {
                        const int j = 4 * (q0 + q);         // (padded cells hold od = 0: thin)
                        if (q0 + q < NQ) quad_indices(od[j < NP ? j : 0], od[j + 1 < NP ? j + 1 : 0], od[j + 2 < NP ? j + 2 : 0], od[j + 3 < NP ? j + 3 : 0], bpade, ig + 4 * q);
                        else ig[4 * q] = ig[4 * q + 1] = ig[4 * q + 2] = ig[4 * q + 3] = 0;
                    }
#pragma unroll
                    for (int q = 0; q < QC; q++) {
                        if (q0 + q < NQ) {
                            scr4 c;
#pragma unroll
                            for (int kk = 0; kk < 4; kk++) {
                                const int j = 4 * (q0 + q) + kk;
                                c.v[kk] = od[j < NP ? j : 0] <= 0.06 ? (scr_t)od[j < NP ? j : 0] : -(scr_t)ig[4 * q + kk];
                            }
                            if (incol) scr_store(W.scr[S_CODE], so0 + (q0 + q) * qstride, c);
                        }
                    }
                }
                if (cloudy) {
                    double odc[GC], tg[GC];
#pragma unroll
                    for (int k = 0; k < GC; k++) odc[k] = odcld;
                    if constexpr (CLOUD == 3 || CLOUD == CL_SHARE) {
#pragma unroll
                        for (int k = 0; k < GC; k++) odc[k] = ((gbits >> (4 * q0 + k)) & 1u) ? odcld : 0.0;
                    }
                    if constexpr (CLOUD == 2) {
#pragma unroll
                        for (int q = 0; q < QC; q++) {
                            if (q0 + q < NQ) {
                                const double2 *po = reinterpret_cast<const double2 *>(W.odg + (so0 + (q0 + q) * qstride) * 4);
                                const double2 a = po[0], b = po[1];
                                odc[4 * q] = a.x; odc[4 * q + 1] = a.y; odc[4 * q + 2] = b.x; odc[4 * q + 3] = b.y;
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < GC; k++) {
                        const int j = 4 * q0 + k;
                        if (j < NP) {
                            const bool p3 = !(od[j] + odc[k] < 0.06) && !(od[j] <= 0.06);
                            int igk = 0;
                            if constexpr (REUSE) igk = p3 ? ig[k] : 0;
                            else { if (j < ng && p3) igk = lut_index(od[j], bpade); }
                            tg[k] = tau_tbl[igk];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < QC; q++) {
                        if (q0 + q < NQ) {
                            scr4 c;
                            double odtot[4];
                            bool tk[4];             // the total optical depth takes the table (a padded cell never does)
                            int it[4];
#pragma unroll
                            for (int kk = 0; kk < 4; kk++) {
                                const int k = 4 * q + kk, j = 4 * (q0 + q) + kk;
                                const bool p1 = od[j] + odc[k] < 0.06;
                                const bool p3 = !p1 && !(od[j] <= 0.06);
                                odtot[kk] = (p3 ? tg[k] : od[j]) + odc[k];
                                tk[kk] = j < ng && !p1;
                            }
                            quad_indices(odtot[0], odtot[1], odtot[2], odtot[3], tk[0], tk[1], tk[2], tk[3], bpade, it);
#pragma unroll
                            for (int kk = 0; kk < 4; kk++) {
                                const int j = 4 * (q0 + q) + kk;
                                c.v[kk] = j < ng ? (tk[kk] ? -(scr_t)it[kk] : (scr_t)odtot[kk]) : (scr_t)0;
                            }
                            if (incol) scr_store(W.scr[S_CODET], so0 + (q0 + q) * qstride, c);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_optics (k_layer's machinery with CLOUD = CL_OPTICS): what k_layer forms for a (layer, column) and then codes away, stored in the
// caller's arrays instead - taumol's gas optical depth per g-point (rows_eval_band from tau0 = 0: no aerosol, no secdiff, no clamp) and
// Planck fraction per g-point (src/rrtmg_lw_taumol.f90), setcoef's Planck integrals per band (src/rrtmg_lw_setcoef.f90:173-269, band 16
// as in a broadband call).  Every value is written once: streaming stores through a descriptor whose range is the batch's part of the
// output row, so that a thread past the last column (offset out of range) stores nothing without a branch (profiles/round5_exec_hazard.md).
// ------------------------------------------------------------------------------------------------
constexpr int CL_OPTICS = 4;

__device__ __forceinline__ void opt_store(double *row, unsigned bytes, unsigned off8, double v)
{
    typedef unsigned int u32x2o __attribute__((ext_vector_type(2)));
    u32x2o x;
    __builtin_memcpy(&x, &v, 8);
    __builtin_amdgcn_raw_buffer_store_b64(x, __builtin_amdgcn_make_buffer_rsrc(row, 0, (int)bytes, 0x00020000), (int)off8, 0, 2);    // (aux 2: nt)
}

// integrated Planck function of one band's totplnk row at temperature t: setcoef :190-205, in the sweeps' arithmetic (planck_at)
__device__ __forceinline__ double planck_band(const double *tp, double t)
{
    const double x = t - 159.;
    const int ind = clampi((int)x, 1, 180);
    const double f = x - (double)ind;
    return fma(f, tp[ind] - tp[ind - 1], tp[ind - 1]);
}

// taug and fracs of band B for one (layer, column); off8: the thread's byte offset in an output row (out of range past the last column)
template <int B, bool LOWER, int N, bool LDS>
__device__ __forceinline__ void optics_cells(const DevTables &T, const Workspace &W, const LayerArgs &a, const LayerCoef &C, __amdgpu_buffer_rsrc_t kt,
                                             const double2 *lds, const Rows<N> &rw, int lay, unsigned off8, const OptOut &o)
{
    constexpr Region R = LOWER ? BT<B>::lo : BT<B>::up;
    constexpr int ng = BT<B>::ng, NP = 4 * band_nquad(B), G0 = band_g0(B);
    const size_t nct = (size_t)a.nct, gstride = nct * (size_t)W.nlay;
    const unsigned bytes = (unsigned)a.ncol * 8u;
    const size_t row0 = (size_t)a.col0 + nct * (size_t)(lay - 1) + gstride * (size_t)G0;
    double od[NP];
    rows_eval_band<B, LOWER, N, LDS>(kt, lds, rw, 0.0, od);
#pragma unroll
    for (int j = 0; j < ng; j++) opt_store(o.taug + row0 + gstride * (size_t)j, bytes, off8, od[j]);
    __builtin_amdgcn_sched_barrier(0);          // (the optical depths are stored before the fraction rows are loaded)
    // Planck fractions: the sweeps' rows (sweep_stage_band / frac_row) - fracrefa below laytrop, fracrefb above (band 6: fracrefa, bands
    // 12 and 15: none), interpolated in the mixture where the region has a binary key (taumol :556-561, :692-693) with the weight fs in
    // full precision (the sweeps carry it in 28 bits: Rows::fw)
    constexpr bool FROM_A = LOWER || R.frac_from_a;
    const BandLayout &L = T.band[B - 1];
    const int base = FROM_A ? L.fracrefa : L.fracrefb;
    const bool have = R.key != K_ZERO && base >= 0;         // (uniform)
    unsigned r0 = have ? (unsigned)base : 0u;
    double fs = 0.0;
    if constexpr (R.key == K_BINARY) {
        const Spec sp = spec_calc(C.f[F_COLH2O + R.a], T.refrat[B - 1][R.planck_slot], C.f[F_COLH2O + R.b], LOWER ? 8. : 4., T.oneminus);
        r0 += (unsigned)(sp.js - 1) * (unsigned)ng;
        fs = sp.fs;
    }
#pragma unroll
    for (int p = 0; p < ng / 2; p++) {
        double2 f = make_double2(0.0, 0.0);
        if (have) {
            const double2 f0 = ld2(kt, r0 + 2u * (unsigned)p);
            f = f0;
            if constexpr (R.key == K_BINARY) {
                const double2 f1 = ld2(kt, r0 + (unsigned)ng + 2u * (unsigned)p);
                f.x = fma(fs, f1.x - f0.x, f0.x);
                f.y = fma(fs, f1.y - f0.y, f0.y);
            }
        }
        opt_store(o.fracs + row0 + gstride * (size_t)(2 * p), bytes, off8, f.x);
        opt_store(o.fracs + row0 + gstride * (size_t)(2 * p + 1), bytes, off8, f.y);
    }
}

// band B of one (layer, column) in k_optics: layer_band's row lists and staging offsets, optics_cells in place of band_cells
template <int B, class WN, int BASE_LO, int BASE_UP>
__device__ __forceinline__ void optics_band(const DevTables &T, const Workspace &W, const LayerArgs &a, const LayerCoef &C, __amdgpu_buffer_rsrc_t kt,
                                            const double2 *lds, int jp0, int im0, bool ok, bool lower, int lay, int col, bool incol, const OptOut &o)
{
    unsigned delta[NROLE];
    const bool use_lds = __builtin_amdgcn_ballot_w64(!ok) == 0ull;          // wave-uniform: every cell of the wave lies in the staged window
    const unsigned off8 = incol ? (unsigned)col * 8u : 0x80000000u;        // (a select, not a branch)
    if (lower) {
        constexpr int N = region_nrows(BT<B>::lo, true);
        Rows<N> rw;
        rows_prep<B, true, N>(T, C, rw);
        if (use_lds) {
            band_delta<B, true, WN, BASE_LO>(T, jp0, im0, delta);
            rows_to_lds<B, true, N>(rw, delta);
            optics_cells<B, true, N, true>(T, W, a, C, kt, lds, rw, lay, off8, o);
        } else {
            optics_cells<B, true, N, false>(T, W, a, C, kt, lds, rw, lay, off8, o);
        }
    } else {
        constexpr int N = region_nrows(BT<B>::up, false);
        Rows<N> rw;
        rows_prep<B, false, N>(T, C, rw);
        if constexpr (B == 16) {
            // The reference sets nspb(16) = 0 (src/rrtmg_lw_init.f90:228), so taugb16's upper-atmosphere indices
            // ind0 = ((jp-13)*5 + (jt-1))*nspb(16) + 1 and ind1 (src/rrtmg_lw_taumol.f90, band 16 upper loop) are 1 whatever
            // the layer: its taug reads absb rows 1 and 2 with the layer's four weights.  This entry returns the reference's
            // taug; the solver's k_layer indexes the table by (jp, jt) (optical depths ~1e-8 there: no flux-level difference).
            const unsigned tab = (unsigned)T.band[B - 1].absb, ng = (unsigned)BT<B>::ng;
            rw.off[0] = tab; rw.off[1] = tab + ng; rw.off[2] = tab; rw.off[3] = tab + ng;
            optics_cells<B, false, N, false>(T, W, a, C, kt, lds, rw, lay, off8, o);
        } else if (use_lds) {
            band_delta<B, false, WN, BASE_UP>(T, jp0, im0, delta);
            rows_to_lds<B, false, N>(rw, delta);
            optics_cells<B, false, N, true>(T, W, a, C, kt, lds, rw, lay, off8, o);
        } else {
            optics_cells<B, false, N, false>(T, W, a, C, kt, lds, rw, lay, off8, o);
        }
    }
}

#ifndef RRLW_LAYER_WAVES
#define RRLW_LAYER_WAVES 3        // waves per SIMD k_layer is compiled for (168 VGPRs; three workgroups of 256 threads and 53 KB of LDS per CU)
#endif

// workgroup-level state of the LDS staging: the staged region (lower / upper atmosphere), first pressure plane and first minor-gas
// temperature slice, this thread's place in the copy loops, and whether this thread's cell lies inside the staged window
struct LayerWg { double2 *lds; int jp0, im0, tid, nth, pc; bool lower, ok; };      // pc: the thread's column of the batch (caller arrays; `col` is its position)

// all cells of band B for one (layer, column); BASE_LO / BASE_UP: where the band's tables start in the staging buffer of its pass
template <int B, int CLOUD, class WN, int BASE_LO, int BASE_UP>
__device__ __forceinline__ void layer_band(const DevTables &T, const Workspace &W, const LayerArgs &a, const LayerCoef &C,
                                           __amdgpu_buffer_rsrc_t kt, const LayerWg &wg, bool lower, int lay, int col, bool incol, int cloudy,
                                           const unsigned (&mw)[MASK_WORDS])
{
    STAMP(4);                                                                   // (cells of the previous band)
    unsigned delta[NROLE];
#pragma unroll
    for (int r = 0; r < NROLE; r++) delta[r] = 0u;
    const bool use_lds = __builtin_amdgcn_ballot_w64(!wg.ok) == 0ull;       // wave-uniform: every cell of the wave lies in the staged window
    const size_t ncb = W.ncolb, gcx = (size_t)a.col0 + wg.pc;
    double odcld = 0.0;
    if constexpr (CLOUD == 1 || CLOUD == 3 || CLOUD == CL_SHARE) { if (cloudy) odcld = W.odcld[((size_t)(B - 1) * W.nlay + (lay - 1)) * ncb + col]; }   // (written for cloudy layers only)
    const double secdiff = W.percol[(size_t)(PC_SECDIFF + B - 1) * ncb + col];
    const double taua = col_load(a.tauaer + (size_t)a.col0 + (size_t)a.nct * ((lay - 1) + (size_t)W.nlay * (B - 1)), (unsigned)wg.pc * 8u);
    unsigned gbits = 0u;
    if constexpr (CLOUD == 3 || CLOUD == CL_SHARE) {
        // the band's bits of the sub-column mask: the one or two words that hold them, read here (all five held from the top of the kernel
        // ended up in scratch memory)
        (void)mw;
        constexpr int g0 = band_g0(B), ng = BT<B>::ng, w0 = g0 >> 5, w1 = (g0 + ng - 1) >> 5;
        if (cloudy) {
            const unsigned *mrow = W.mask + (size_t)(lay - 1) * W.mask_stride + W.mask_col0 + gcx;
            const unsigned long long lo = mrow[(size_t)w0 * W.nlay * W.mask_stride];
            const unsigned long long hi = w1 != w0 ? mrow[(size_t)w1 * W.nlay * W.mask_stride] : 0u;
            gbits = (unsigned)(((lo | (hi << 32)) >> (g0 & 31)) & ((1ull << ng) - 1ull));
        }
    }
    if (lower) {
        constexpr int N = region_nrows(BT<B>::lo, true);
        Rows<N> rw;
        rows_prep<B, true, N>(T, C, rw);
        if (use_lds) {
            band_delta<B, true, WN, BASE_LO>(T, wg.jp0, wg.im0, delta);
            rows_to_lds<B, true, N>(rw, delta);
            STAMP(2);
            band_cells<B, CLOUD, true, N, true>(T, W, kt, wg.lds, rw, lay, col, incol, secdiff, taua, cloudy, odcld, gbits);
        } else {
            band_cells<B, CLOUD, true, N, false>(T, W, kt, wg.lds, rw, lay, col, incol, secdiff, taua, cloudy, odcld, gbits);
        }
    } else {
        constexpr int N = region_nrows(BT<B>::up, false);
        Rows<N> rw;
        rows_prep<B, false, N>(T, C, rw);
        if (use_lds) {
            band_delta<B, false, WN, BASE_UP>(T, wg.jp0, wg.im0, delta);
            rows_to_lds<B, false, N>(rw, delta);
            STAMP(2);
            band_cells<B, CLOUD, false, N, true>(T, W, kt, wg.lds, rw, lay, col, incol, secdiff, taua, cloudy, odcld, gbits);
        } else {
            band_cells<B, CLOUD, false, N, false>(T, W, kt, wg.lds, rw, lay, col, incol, secdiff, taua, cloudy, odcld, gbits);
        }
    }
}

// The staging passes: every band once, in evaluation order (bands that are the only users of some setcoef quantity - pavel, broadening
// gases, O2, halocarbons, CO - first, the bands with the longest row lists last: their register peak then meets fewer live quantities).
// A pass must fit the staging buffer in both regions of the atmosphere (static_assert in stage_pass).
// (Measured against these four passes, 24.3 - 24.6 ms, in round 3: one staging round per band as before that round 25.9, three passes with
// 384-thread workgroups and a 9 000-double buffer 40.6 against 23.6, one pass with one 768-thread workgroup per CU 25.6 -
// profiles/round3_k_layer_stamps.md.)
#ifdef RRLW_G256
using LayerPasses = std::tuple<BandList<1, 2, 11, 15, 6>, BandList<8, 10, 14, 16>, BandList<12>, BandList<13>, BandList<4, 9>, BandList<7>, BandList<3>, BandList<5>>;
#else
using LayerPasses = std::tuple<BandList<1, 2, 11, 15, 6, 8, 10, 14, 16, 12, 13>, BandList<4, 9>, BandList<7, 3>, BandList<5>>;
#endif
// ... and with the wide window (five planes, ten minor-gas slices: the tables of the binary-key bands take 5/3 of the space)
#ifdef RRLW_G256
using LayerPassesWide = LayerPasses;
#else
using LayerPassesWide = std::tuple<BandList<1, 2, 11, 15, 6, 8, 10, 14, 16, 13>, BandList<12, 4>, BandList<9>, BandList<7>, BandList<3>, BandList<5>>;
#endif

template <class PL, class WN, int CLOUD, int... I>
__device__ __forceinline__ void pass_run(std::integer_sequence<int, I...>, const DevTables &T, const Workspace &W, const LayerArgs &a,
                                         const LayerCoef &C, __amdgpu_buffer_rsrc_t kt, const LayerWg &wg, bool lower, int lay, int col, bool incol,
                                         int cloudy, const unsigned (&mw)[MASK_WORDS], unsigned bmask, const OptOut &o)
{
    // (a workgroup that holds none of the pass's bands - the bands of a small batch spread over several - leaves the pass alone: uniform)
    constexpr unsigned passmask = ((1u << (PL::b[I] - 1)) | ...);
    if ((bmask & passmask) == 0u) return;
    // the pass's tables -> LDS; the barriers are reached by every thread of the workgroup
    STAMP(4);
    lds_barrier();                      // the previous pass's readers are done with the staging buffer
    STAMP(0);
    if (wg.lower) stage_pass<PL, true, WN>(T, kt, wg.lds, wg.jp0, wg.im0, wg.tid);
    else stage_pass<PL, false, WN>(T, kt, wg.lds, wg.jp0, wg.im0, wg.tid);
    lds_barrier();
    STAMP(1);
    if constexpr (CLOUD == CL_OPTICS) {
        (((bmask >> (PL::b[I] - 1)) & 1u
              ? optics_band<PL::b[I], WN, pass_base<PL, true, WN, I>(), pass_base<PL, false, WN, I>()>(T, W, a, C, kt, wg.lds, wg.jp0, wg.im0, wg.ok, lower, lay, col, incol, o)
              : (void)0), ...);
    } else {
        (((bmask >> (PL::b[I] - 1)) & 1u
              ? layer_band<PL::b[I], CLOUD, WN, pass_base<PL, true, WN, I>(), pass_base<PL, false, WN, I>()>(T, W, a, C, kt, wg, lower, lay, col, incol, cloudy, mw)
              : (void)0), ...);
    }
}
template <int CLOUD, class WN, class... PLs>
__device__ __forceinline__ void passes_run(std::tuple<PLs...> *, const DevTables &T, const Workspace &W, const LayerArgs &a,
                                           const LayerCoef &C, __amdgpu_buffer_rsrc_t kt, const LayerWg &wg, bool lower, int lay, int col, bool incol,
                                           int cloudy, const unsigned (&mw)[MASK_WORDS], unsigned bmask, const OptOut &o)
{
    (pass_run<PLs, WN, CLOUD>(std::make_integer_sequence<int, PLs::n>{}, T, W, a, C, kt, wg, lower, lay, col, incol, cloudy, mw, bmask, o), ...);
}

// One workgroup's work: the cells of window `bx` (256 consecutive positions) in layer `by` + 1.  WIDE = 0: the narrow staging window; a
// workgroup whose cells do not fit it leaves its (window, layer) in W.wide and returns.  WIDE = 1: the wide window (k_layer<.., 1> walks
// that list).
template <bool GCM, int CLOUD, int WIDE>
__device__ __forceinline__ void layer_cells(const DevTables &T, const Workspace &W, const GcmIn &g, const ColIn &c, const LayerArgs &a, double2 *s_tab, int *s_wg,
                                            int bx, int by, unsigned bmask, bool lists, const OptOut &o)
{
    const int colr = bx * LAYER_BLOCK + threadIdx.x;
    const bool incol = colr < a.ncol;
    const int col = incol ? colr : a.ncol - 1;      // threads past the end shadow the last column (they take part in the staging and the barriers)
    const int lay = by + 1;
    const int pc = pcol(W, col);                    // the column this position holds (k_colsort)
    const size_t gc = (size_t)a.col0 + pc;
    const int nct = a.nct;
    const size_t gi = gc + (size_t)nct * (lay - 1);
    const double *S = T.stat;
    const double *preflog = S + T.sl.preflog, *tref = S + T.sl.tref;
    const double amd = 28.9660, amw = 18.0160, avogad = 6.02214199e+23, grav = 9.8066;
    const double stpfac = 296. / 1013.;

    // The narrow launch decides FIRST whether the workgroup's cells fit its window - from the layer's pressures and temperatures alone -
    // and a workgroup that leaves for the wide launch has then read two of its fifteen input rows and computed nothing else (on a
    // terrain-following grid nine workgroups in ten leave: profiles/round5_orography.md).  The others go on as before; what they have found
    // of the window stays in s_wg.
    bool early = false;
    if constexpr (WIDE == 0 && GCM && HAVE_WIDE) {
        if (W.wide) {           // (uniform)
            early = true;
            const size_t ro = (size_t)a.col0 + (size_t)nct * (lay - 1);
            const double pe = col_load(g.play + ro, (unsigned)pc * 8u), te = col_load(g.tlay + ro, (unsigned)pc * 8u);
            const int jpe = clampi((int)(36. - 5 * (log(pe) + 0.04)), 1, 58);
            const int ime = min(18, max(1, (int)fdiv(te - 180.8, 7.2)));
            const bool lowe = lay <= W.laytrop[col];
            if (threadIdx.x == 0) { s_wg[0] = lowe ? 1 : 0; s_wg[1] = 99; s_wg[2] = 99; s_wg[3] = 0; s_wg[4] = 0; }
            __syncthreads();
            const bool in = lowe == (s_wg[0] != 0);
            int jlo = in ? jpe : 99, ilo = in ? ime : 99, jhi = in ? jpe : 0, ihi = in ? ime : 0;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                jlo = min(jlo, __shfl_xor(jlo, o, 64)); ilo = min(ilo, __shfl_xor(ilo, o, 64));
                jhi = max(jhi, __shfl_xor(jhi, o, 64)); ihi = max(ihi, __shfl_xor(ihi, o, 64));
            }
            if ((threadIdx.x & 63) == 0) { atomicMin(&s_wg[1], jlo); atomicMin(&s_wg[2], ilo); atomicMax(&s_wg[3], jhi); atomicMax(&s_wg[4], ihi); }
            __syncthreads();
            const int jp0 = s_wg[1], im0 = min(s_wg[2], 20 - WinNarrow::MW);
            if (s_wg[3] - jp0 > WinNarrow::NPL - 2 || s_wg[4] - im0 > WinNarrow::MW - 2) {
                if (threadIdx.x == 0 && lists) W.wide[2 + atomicAdd(&W.wide[0], 1)] = by * ((a.ncol + LAYER_BLOCK - 1) / LAYER_BLOCK) + bx;     // (one of the pair's workgroups lists it)
                return;
            }
        }
    }

    double pavel, tavel, coldry, wbrodl, w1, w2, w3, w4, w5, w6, w7;
    LayerCoef C;
    if (GCM) {
        const size_t ro = (size_t)a.col0 + (size_t)nct * (lay - 1);      // the layer's row of a (ncol, nlay) array (uniform)
        const unsigned o8 = (unsigned)pc * 8u;
        pavel = col_load(g.play + ro, o8);
        tavel = col_load(g.tlay + ro, o8);
        const double pz_lo = col_load(g.plev + ro, o8), pz_hi = col_load(g.plev + ro + nct, o8);
        w1 = col_load(g.h2ovmr + ro, o8); w2 = col_load(g.co2vmr + ro, o8); w3 = col_load(g.o3vmr + ro, o8); w4 = col_load(g.n2ovmr + ro, o8);
        w5 = 0.0; w6 = col_load(g.ch4vmr + ro, o8); w7 = col_load(g.o2vmr + ro, o8);
        const double amm = (1. - w1) * amd + w1 * amw;
        coldry = fdiv((pz_lo - pz_hi) * 1.e3 * avogad, 1.e2 * grav * amm * (1. + w1));
        double summol = 0.0;
        summol = summol + w2; summol = summol + w3; summol = summol + w4;
        summol = summol + w5; summol = summol + w6; summol = summol + w7;
        wbrodl = coldry * (1. - summol);
        w1 = coldry * w1; w2 = coldry * w2; w3 = coldry * w3; w4 = coldry * w4;
        w5 = coldry * w5; w6 = coldry * w6; w7 = coldry * w7;
        C.f[F_WX1] = coldry * col_load(g.ccl4vmr + ro, o8) * 1.e-20;
        C.f[F_WX2] = coldry * col_load(g.cfc11vmr + ro, o8) * 1.e-20;
        C.f[F_WX3] = coldry * col_load(g.cfc12vmr + ro, o8) * 1.e-20;
        C.f[F_WX4] = coldry * col_load(g.cfc22vmr + ro, o8) * 1.e-20;
    } else {
        pavel = c.pavel[gi];
        tavel = c.tavel[gi];
        coldry = c.coldry[gi];
        wbrodl = c.wbrodl[gi];
        const size_t wi = gc + (size_t)nct * 7 * (lay - 1);       // wkl (ncol,7,nlayers)
        w1 = c.wkl[wi]; w2 = c.wkl[wi + (size_t)nct]; w3 = c.wkl[wi + (size_t)nct * 2];
        w4 = c.wkl[wi + (size_t)nct * 3]; w5 = c.wkl[wi + (size_t)nct * 4]; w6 = c.wkl[wi + (size_t)nct * 5];
        w7 = c.wkl[wi + (size_t)nct * 6];
        const size_t xi = gc + (size_t)nct * 4 * (lay - 1);       // wx (ncol,4,nlayers)
        C.f[F_WX1] = c.wx[xi]; C.f[F_WX2] = c.wx[xi + (size_t)nct];
        C.f[F_WX3] = c.wx[xi + (size_t)nct * 2]; C.f[F_WX4] = c.wx[xi + (size_t)nct * 3];
    }

    // (the Planck functions of setcoef :173-269 are formed by the sweeps, which need them per band and level)
    // pressure / temperature interpolation: setcoef :276-306
    const double plog = log(pavel);
    const int jp = clampi((int)(36. - 5 * (plog + 0.04)), 1, 58);
    const double fp = 5. * (preflog[jp - 1] - plog);
    const double dt0 = fdiv(tavel - tref[jp - 1], 15.), dt1 = fdiv(tavel - tref[jp], 15.);
    const int jt = clampi((int)(3. + dt0), 1, 4);
    const double ft = dt0 - (double)(jt - 3);
    const int jt1 = clampi((int)(3. + dt1), 1, 4);
    const double ft1 = dt1 - (double)(jt1 - 3);
    const double water = fdiv(w1, coldry);
    const double scalefac = fdiv(pavel * stpfac, tavel);
    int indself = 1, indfor, indminor;
    double forfac, forfrac, selffac, selffrac = 0.0, factor;
    if (!(plog <= 4.56)) {            // :312-334
        forfac = fdiv(scalefac, 1. + water);
        factor = fdiv(332.0 - tavel, 36.0);
        indfor = min(2, max(1, (int)factor));
        forfrac = factor - (double)indfor;
        selffac = water * forfac;
        factor = fdiv(tavel - 188.0, 7.2);
        indself = min(9, max(1, (int)factor - 7));
        selffrac = factor - (double)(indself + 7);
    } else {                          // :369-377
        forfac = fdiv(scalefac, 1. + water);
        factor = fdiv(tavel - 188.0, 36.0);
        indfor = 3;
        forfrac = factor - 1.0;
        selffac = water * forfac;
    }
    factor = fdiv(tavel - 180.8, 7.2);
    indminor = min(18, max(1, (int)factor));
    C.f[F_MINORFRAC] = factor - (double)indminor;
    C.f[F_SCALEMINOR] = fdiv(pavel, tavel);
    C.f[F_SCALEMINORN2] = C.f[F_SCALEMINOR] * fdiv(wbrodl, coldry + w1);
    double colh2o = 1.e-20 * w1, colco2 = 1.e-20 * w2, colo3 = 1.e-20 * w3, coln2o = 1.e-20 * w4;
    double colco = 1.e-20 * w5, colch4 = 1.e-20 * w6, colo2 = 1.e-20 * w7;
    if (colco2 == 0.) colco2 = 1.e-32 * coldry;
    if (colo3 == 0.) colo3 = 1.e-32 * coldry;
    if (coln2o == 0.) coln2o = 1.e-32 * coldry;
    if (colco == 0.) colco = 1.e-32 * coldry;
    if (colch4 == 0.) colch4 = 1.e-32 * coldry;
    const double compfp = 1. - fp;     // :421-429
    C.f[F_FAC10] = compfp * ft;
    C.f[F_FAC00] = compfp * (1. - ft);
    C.f[F_FAC11] = fp * ft1;
    C.f[F_FAC01] = fp * (1. - ft1);
    C.f[F_SELFFAC] = colh2o * selffac;
    C.f[F_FORFAC] = colh2o * forfac;
    C.f[F_SELFFRAC] = selffrac;
    C.f[F_FORFRAC] = forfrac;
    C.f[F_COLH2O] = colh2o; C.f[F_COLCO2] = colco2; C.f[F_COLO3] = colo3; C.f[F_COLN2O] = coln2o;
    C.f[F_COLCO] = colco; C.f[F_COLCH4] = colch4; C.f[F_COLO2] = colo2; C.f[F_COLBRD] = 1.e-20 * wbrodl;
    C.f[F_COLDRY] = coldry;
    C.f[F_PAVEL] = pavel;
    C.jp = jp; C.jt = jt; C.jt1 = jt1; C.indself = indself; C.indfor = indfor; C.indminor = indminor;

    // "lower atmosphere" for taumol is lay <= laytrop (the count of layers with ln p > 4.56), :312-313
    const bool lower = lay <= W.laytrop[col];
    int cloudy = 0;
    // (threads past the last column never take the cloudy branches: nothing of theirs is stored, and with them no lane of a divergent
    // region skips the `if (incol)` at its end - the construct of profiles/round5_exec_hazard.md)
    if ((CLOUD >= 1 && CLOUD <= 3) || CLOUD == CL_SHARE) cloudy = incol ? (W.cflag[(size_t)lay * W.ncolb + col] & 1) : 0;
    if constexpr (CLOUD == CL_OPTICS) {
        // setcoef :173-269 for the bands of this workgroup: the layer's Planck integral and that of the level above it; the layer-1 threads
        // add level 0 and the surface terms k_colprep has formed for the sweeps (plankbnd with semiss, its d/dT with idrv = 1)
        const size_t nlv = (size_t)W.nlay, ro = (size_t)a.col0 + (size_t)nct * (lay - 1);
        const unsigned o8 = (unsigned)pc * 8u, off8 = incol ? (unsigned)col * 8u : 0x80000000u, bytes = (unsigned)a.ncol * 8u;
        const double tz_up = GCM ? col_load(g.tlev + ro + nct, o8) : c.tz[gc + (size_t)nct * lay];
        const double tz_lo = lay == 1 ? (GCM ? col_load(g.tlev + ro, o8) : c.tz[gc]) : 0.0;
        for (int b = 0; b < NBND; b++) {
            if (!((bmask >> b) & 1u)) continue;                                  // (uniform)
            const double *tp = S + T.sl.totplnk + 181 * b;
            if (o.planklay) opt_store(o.planklay + ro + (size_t)nct * nlv * b, bytes, off8, planck_band(tp, tavel));
            if (o.planklev) {
                const size_t lv0 = (size_t)a.col0 + (size_t)nct * (nlv + 1) * b;
                opt_store(o.planklev + lv0 + (size_t)nct * lay, bytes, off8, planck_band(tp, tz_up));
                if (lay == 1) opt_store(o.planklev + lv0, bytes, off8, planck_band(tp, tz_lo));
            }
            if (lay == 1) {
                if (o.plankbnd) opt_store(o.plankbnd + a.col0 + (size_t)nct * b, bytes, off8, W.percol[(size_t)(PC_PLANKBND + b) * W.ncolb + col]);
                if (o.dplankbnd && a.idrv == 1) opt_store(o.dplankbnd + a.col0 + (size_t)nct * b, bytes, off8, W.percol[(size_t)(PC_DPLANKBND + b) * W.ncolb + col]);
            }
        }
    }
    // wave-uniform descriptor of the packed k tables (built from kernel arguments only)
    const __amdgpu_buffer_rsrc_t kt = __builtin_amdgcn_make_buffer_rsrc((void *)T.ktab, 0, a.ktab_bytes, 0x00020000);
    const unsigned mw[MASK_WORDS] = {};
#ifdef RRLW_LAYER_STAMPS
    if ((threadIdx.x & 63) == 0) { for (int i = 0; i < NSTAMP; i++) s_stamp[(threadIdx.x >> 6) * (NSTAMP + 1) + i] = 0ull; }
    STAMP(-1);
#endif
    // staging window of the workgroup: the region of its first thread, the smallest jp and the smallest indminor among the cells of that region
    for (int i = threadIdx.x; i < NRATCHI; i += LAYER_BLOCK) s_ratchi[i] = S[T.sl.rat + i];
    if (!early) {
        if (threadIdx.x == 0) { s_wg[0] = lower ? 1 : 0; s_wg[1] = 99; s_wg[2] = 99; s_wg[3] = 0; s_wg[4] = 0; }
        __syncthreads();
    }
    LayerWg wg;
    wg.lds = s_tab; wg.tid = threadIdx.x; wg.nth = blockDim.x; wg.pc = pc;
    wg.lower = s_wg[0] != 0;
    // (one wave-level reduction per quantity, then one LDS atomic per wave: 256 atomics on one address serialise)
    if (!early) {
        const bool in = lower == wg.lower;
        int jlo = in ? jp : 99, ilo = in ? indminor : 99, jhi = in ? jp : 0, ihi = in ? indminor : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            jlo = min(jlo, __shfl_xor(jlo, o, 64)); ilo = min(ilo, __shfl_xor(ilo, o, 64));
            jhi = max(jhi, __shfl_xor(jhi, o, 64)); ihi = max(ihi, __shfl_xor(ihi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(&s_wg[1], jlo); atomicMin(&s_wg[2], ilo); atomicMax(&s_wg[3], jhi); atomicMax(&s_wg[4], ihi); }
    }
    __syncthreads();
    wg.jp0 = s_wg[1];
    using WN = std::conditional_t<WIDE != 0, WinWide, WinNarrow>;
    wg.im0 = min(s_wg[2], 20 - WN::MW);                     // (the window ends with the table's last slice at the latest)
    wg.ok = lower == wg.lower && (unsigned)(jp - wg.jp0) <= (unsigned)(WN::NPL - 2) && (unsigned)(indminor - wg.im0) <= (unsigned)(WN::MW - 2);
    STAMP(5);                       // set-up of the workgroup's staging window
    passes_run<CLOUD, WN>(static_cast<std::conditional_t<WIDE != 0, LayerPassesWide, LayerPasses> *>(nullptr), T, W, a, C, kt, wg, lower, lay, col, incol, cloudy, mw, bmask, o);
#ifdef RRLW_LAYER_STAMPS
    STAMP(4);
    if ((threadIdx.x & 63) == 0) {
        for (int i = 0; i < NSTAMP; i++) atomicAdd(&g_stamps[i], s_stamp[(threadIdx.x >> 6) * (NSTAMP + 1) + i]);
        atomicAdd(&g_stamps[NSTAMP], 1ull);
    }
#endif
}

// WIDE = 0: grid (windows, layers), one workgroup per (window, layer).  WIDE = 1: grid (windows x layers); workgroup i takes pair i of the
// list the narrow launch left in W.wide = {count, -, pair ..} and leaves at once when there is none (a (window, layer) grid of
// workgroups that read one word and leave costs ~25 us per 250 000 columns; a fixed grid of workgroups that LOOP over the list spills
// 151 registers: everything derived from the kernel's arguments stays live round the loop).  The count is cleared on the stream in front
// of the narrow launch (driver.hip: run_layer).
template <bool GCM, int CLOUD, int WIDE>
__device__ __forceinline__ void layer_grid(const DevTables &T, const Workspace &W, const GcmIn &g, const ColIn &c, const LayerArgs &a, double2 *s_tab, int *s_wg,
                                           const OptOut &o)
{
    // the bands this workgroup takes: those of the call's range, of its part where the bands of a small batch are spread over several workgroups
    const int part = WIDE == 0 ? blockIdx.z : blockIdx.y;
    unsigned bmask = ((a.iend >= 32 ? 0u : (1u << a.iend)) - 1u) & ~((1u << (a.istart - 1)) - 1u);
    if (a.nparts > 1) bmask &= a.partmask[part];
    if constexpr (WIDE == 0) {
        layer_cells<GCM, CLOUD, 0>(T, W, g, c, a, s_tab, s_wg, blockIdx.x, blockIdx.y, bmask, part == 0, o);
    } else {
        const int n = __builtin_amdgcn_readfirstlane(W.wide[0]), gx = (a.ncol + LAYER_BLOCK - 1) / LAYER_BLOCK;
        if ((int)blockIdx.x >= n) return;
        const int item = __builtin_amdgcn_readfirstlane(W.wide[2 + blockIdx.x]);
        layer_cells<GCM, CLOUD, 1>(T, W, g, c, a, s_tab, s_wg, item % gx, item / gx, bmask, false, o);
    }
}
template <bool GCM, int CLOUD, int WIDE>
__global__ __launch_bounds__(LAYER_BLOCK, RRLW_LAYER_WAVES) void k_layer(DevTables T, Workspace W, GcmIn g, ColIn c, LayerArgs a)
{
    __shared__ double2 s_tab[STAGE_DOUBLES / 2];
    __shared__ int s_wg[5];
    layer_grid<GCM, CLOUD, WIDE>(T, W, g, c, a, s_tab, s_wg, OptOut{});
}
// k_optics: the gas-optics entries (rrtmg_lw_hip_gas_optics*) - k_layer's grid, windows, staging passes and table evaluation with the
// outputs of OptOut in place of the cell codes; no cloud, no aerosol.  WIDE as for k_layer.
template <bool GCM, int WIDE>
__global__ __launch_bounds__(LAYER_BLOCK, RRLW_LAYER_WAVES) void k_optics(DevTables T, Workspace W, GcmIn g, ColIn c, LayerArgs a, OptOut o)
{
    __shared__ double2 s_tab[STAGE_DOUBLES / 2];
    __shared__ int s_wg[5];
    layer_grid<GCM, CL_OPTICS, WIDE>(T, W, g, c, a, s_tab, s_wg, o);
}

// ------------------------------------------------------------------------------------------------
// k_codet : the total-optical-depth codes (S_CODET) of the cloudy layers of one sub-column sample from the float64 optical depths
//           k_layer<., CL_SHARE, .> left in W.odg, the sample's mask and its cloud optical depths (k_cloudmc<mask>): the cloudy branch
//           of band_cells, expression for expression - same clamp, same three sub-branches, same table indices -, so that a sample's
//           codes are those k_layer<mcmask> writes for it.  One thread per (position, layer); a layer without a cloudy sub-column
//           leaves at once.  Every cell read was stored: k_layer stores all quads of all layers of the batch's columns.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_codet(DevTables T, Workspace W, int ncol, int col0)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncol) return;
    const int lay = blockIdx.y + 1, nlay = W.nlay;
    const size_t ncb = W.ncolb;
    if (!(W.cflag[(size_t)lay * ncb + col] & 1)) return;
    const size_t gcx = (size_t)col0 + pcol(W, col);
    const double *__restrict__ tau_tbl = T.stat + T.sl.tau_tbl;
    const double bpade = T.bpade;
    const unsigned *mrow = W.mask + (size_t)(lay - 1) * W.mask_stride + W.mask_col0 + gcx;
    const size_t qstride = (size_t)nlay * ncb;
#pragma unroll 1
    for (int B = 1; B <= NBND; B++) {
        const int ng = band_ng(B), g0 = band_g0(B), nq = band_nquad(B);
        const int w0 = g0 >> 5, w1 = (g0 + ng - 1) >> 5;
        const unsigned long long lo = mrow[(size_t)w0 * nlay * W.mask_stride];
        const unsigned long long hi = w1 != w0 ? mrow[(size_t)w1 * nlay * W.mask_stride] : 0u;
        const unsigned gbits = (unsigned)(((lo | (hi << 32)) >> (g0 & 31)) & ((1ull << ng) - 1ull));
        const double odcld = W.odcld[((size_t)(B - 1) * nlay + (lay - 1)) * ncb + col];
        const size_t so0 = ((size_t)band_qstart(B) * nlay + (lay - 1)) * ncb + col;
#pragma unroll 1
        for (int q = 0; q < nq; q++) {
            const double2 *po = reinterpret_cast<const double2 *>(W.odg + (so0 + q * qstride) * 4);
            const double2 a = po[0], b = po[1];
            double od[4] = {a.x, a.y, b.x, b.y}, odc[4], tg[4], odtot[4];
            bool tk[4];
            int it[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = 4 * q + k;
                if (j < ng) { if (!(od[k] >= 0.0)) od[k] = 0.0; }       // rtrn :369
                odc[k] = ((gbits >> j) & 1u) ? odcld : 0.0;
                const bool p3 = !(od[k] + odc[k] < 0.06) && !(od[k] <= 0.06);
                int igk = 0;
                if (j < ng && p3) igk = lut_index(od[k], bpade);
                tg[k] = tau_tbl[igk];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = 4 * q + k;
                const bool p1 = od[k] + odc[k] < 0.06;
                const bool p3 = !p1 && !(od[k] <= 0.06);
                odtot[k] = (p3 ? tg[k] : od[k]) + odc[k];
                tk[k] = j < ng && !p1;
            }
            quad_indices(odtot[0], odtot[1], odtot[2], odtot[3], tk[0], tk[1], tk[2], tk[3], bpade, it);
            scr4 c;
#pragma unroll
            for (int k = 0; k < 4; k++) c.v[k] = 4 * q + k < ng ? (tk[k] ? -(scr_t)it[k] : (scr_t)odtot[k]) : (scr_t)0;
            scr_store(W.scr[S_CODET], so0 + q * qstride, c);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_cloudmc : McICA cloud terms per g-point: cldprmc (src/rrtmg_lw_cldprmc.f90:49-279) followed by the cloud
//             part of rtrnmc's set-up (src/rrtmg_lw_rtrnmc.f90:307-329).  One thread per (column, layer).
//   FROMMASK = false: the sub-column arrays of the reference's McICA argument list, (140,ncol,nlay)
//                     (src/rrtmg_lw_rad.f90:267-298)
//   FROMMASK = true : sub-columns given by the generator's bit mask (k_subcol_*) plus the grid-mean cloud
//                     properties - the same values the generator would have expanded into those arrays
//                     (src/mcica_subcol_gen_lw.f90:664-680).
// ------------------------------------------------------------------------------------------------

template <bool FROMMASK>
__global__ __launch_bounds__(256) void k_cloudmc(DevTables T, Workspace W, McIn m, GcmIn g, int ncol, int col0, int nct,
                                                 int inflag, int iceflag, int liqflag)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncol) return;
    const int lay = blockIdx.y + 1;
    const int nlay = W.nlay;
    const size_t ncb = W.ncolb;
    const size_t gc = (size_t)col0 + pcol(W, col);
    const size_t cl = gc + (size_t)nct * (lay - 1);
    const double *S = T.stat;
    const double *absice1 = S + T.sl.absice1, *absice2 = S + T.sl.absice2, *absice3 = S + T.sl.absice3, *absliq1 = S + T.sl.absliq1;
    const double cldmin = 1.e-20;
    const double radice = FROMMASK ? g.reice[cl] : m.reicmcl[cl];
    const double radliq = FROMMASK ? g.reliq[cl] : m.relqmcl[cl];
    double mciwp = 0.0, mclwp = 0.0;
    unsigned mw[MASK_WORDS] = {};
    if (FROMMASK) {
        mciwp = g.cicewp[cl];
        mclwp = g.cliqwp[cl];
#pragma unroll
        for (int w = 0; w < MASK_WORDS; w++) mw[w] = W.mask[((size_t)w * nlay + (lay - 1)) * W.mask_stride + W.mask_col0 + gc];
    }
    if constexpr (FROMMASK) {
        unsigned anybit = 0u;
#pragma unroll
        for (int w = 0; w < MASK_WORDS; w++) anybit |= (w == MASK_WORDS - 1 && (NGPT & 31)) ? (mw[w] & ((1u << (NGPT & 31)) - 1u)) : mw[w];
        if (anybit == 0u) {       // no cloudy sub-column in this layer (140 = 4 x 32 + 12 bits)
            W.cflag[(size_t)lay * ncb + col] = 0;      // (odcld / efcl of a layer are read only when its flag is set)
            if (lay == 1) W.cflag[(size_t)(nlay + 1) * ncb + col] = 0;
            return;
        }
    }
    // particle-size interpolation positions (band independent): cldprmc :208-262
    int ice_err = 0, liq_err = 0, index_i = 1, index_l = 1;
    double fint_i = 0.0, fint_l = 0.0;
    if (iceflag == 0) { if (radice < 10.0) ice_err = E_ICE_SMALL; }
    else if (iceflag == 1) { if (radice < 13.0 || radice > 130.) ice_err = E_ICE_BOUNDS; }
    else if (iceflag == 2) {
        if (radice < 5.0 || radice > 131.0) ice_err = E_ICE_BOUNDS;
        const double factor = (radice - 2.) / 3.;
        index_i = (int)factor; if (index_i == 43) index_i = 42;
        fint_i = factor - (double)index_i;
        index_i = clampi(index_i, 1, 42);
    } else if (iceflag == 3) {
        if (radice < 5.0 || radice > 140.0) ice_err = E_ICE_GEN_BOUNDS;
        const double factor = (radice - 2.) / 3.;
        index_i = (int)factor; if (index_i == 46) index_i = 45;
        fint_i = factor - (double)index_i;
        index_i = clampi(index_i, 1, 45);
    }
    if (liqflag == 1) {
        if (radliq < 2.5 || radliq > 60.) liq_err = E_LIQ_BOUNDS;
        index_l = (int)(radliq - 1.5);
        if (index_l == 0) index_l = 1;
        if (index_l == 58) index_l = 57;
        fint_l = radliq - 1.5 - (double)index_l;
        index_l = clampi(index_l, 1, 57);
    }
    int err = 0, any = 0, quad = 0;
#pragma unroll 1
    for (int B = 1; B <= NBND; B++) {
        const int ng = band_ng(B), g0 = band_g0(B);
        const double secdiff = W.percol[(size_t)(PC_SECDIFF + B - 1) * ncb + col];
        double ai = 0.0, al = 0.0;         // coefficients of a cell of this band that holds ice / liquid
        if (inflag == 2) {
            if (iceflag == 0) ai = T.absice0[0] + T.absice0[1] / radice;
            else if (iceflag == 1) {
                const int icx = B <= 2 ? B : (B <= 5 ? 3 : (B <= 8 ? 4 : 5));                 // ipat(1:16,1), cldprmc :214-216
                ai = absice1[2 * (icx - 1)] + absice1[2 * (icx - 1) + 1] / radice;
            } else if (iceflag == 2) { const double *t = absice2 + 43 * (B - 1); ai = t[index_i - 1] + fint_i * (t[index_i] - t[index_i - 1]); }
            else if (iceflag == 3) { const double *t = absice3 + 46 * (B - 1); ai = t[index_i - 1] + fint_i * (t[index_i] - t[index_i - 1]); }
            if (liqflag == 0) al = T.absliq0;
            else if (liqflag == 1) { const double *t = absliq1 + 58 * (B - 1); al = t[index_l - 1] + fint_l * (t[index_l] - t[index_l - 1]); }
        }
        const double tband = FROMMASK ? g.taucld[(B - 1) + (size_t)NBND * cl] : 0.0;
        if constexpr (FROMMASK) {
            // every cloudy cell of this band and layer carries the same values (src/mcica_subcol_gen_lw.f90:664-680): one
            // optical depth / emissivity per band; k_layer<..,3,..> and k_sweepz<.,4> combine them with the mask bits
            const unsigned long long lo = mw[g0 >> 5], hi = (g0 >> 5) < MASK_WORDS - 1 ? mw[(g0 >> 5) + 1] : 0u;
            const unsigned bits = (unsigned)(((lo | (hi << 32)) >> (g0 & 31)) & ((1ull << ng) - 1ull));
            double t = tband, od = 0.0, ef = 0.0;
            if (bits) {
                if (mciwp + mclwp >= cldmin || t >= cldmin) {                                 // cldprmc :181-183 with cldfmc = 1
                    if (inflag == 1) err = E_MC_INFLAG1;
                    else if (inflag == 2) {
                        double a_i = 0.0, a_l = 0.0;
                        if (mciwp != 0.0 && iceflag >= 0 && iceflag <= 3) { a_i = ai; if (ice_err && !err) err = ice_err; }      // the first stop in the reference's order
                        if (mclwp != 0.0) {
                            if (liqflag == 0) a_l = al;
                            else if (liqflag == 1) { a_l = al; if (liq_err && !err) err = liq_err; }       // (ice is checked first: cldprmc :204-254)
                        }
                        t = mciwp * a_i + mclwp * a_l;
                    }
                }
                od = secdiff * t;                                                               // rtrnmc :311-317
                ef = (double)(float)(1. - exp(-od));      // rounded as the array path stores it (cfef is float)
                any = 1;
            }
            const size_t o = ((size_t)(B - 1) * nlay + (lay - 1)) * ncb + col;
            W.odcld[o] = od;
            W.efcl[o] = ef;
            continue;
        }
#pragma unroll 1
        for (int qi = 0; qi < (ng + 3) / 4; qi++, quad++) {
            double cf[4], tau[4], ci[4], cw[4];
            if (FROMMASK) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int ig = g0 + 4 * qi + j;
                    const bool on = (4 * qi + j < ng) && ((mw[ig >> 5] >> (ig & 31)) & 1u);
                    cf[j] = on ? 1.0 : 0.0; tau[j] = on ? tband : 0.0; ci[j] = on ? mciwp : 0.0; cw[j] = on ? mclwp : 0.0;
                }
            } else {
                const size_t base = (size_t)(g0 + 4 * qi) + (size_t)NGPT * cl;     // 16-byte aligned: every band starts on an even g
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    if (4 * qi + 2 * h < ng) {              // band sizes are even: a pair is inside the band or outside it
                        const double2 a = *reinterpret_cast<const double2 *>(m.cldfmcl + base + 2 * h);
                        const double2 b = *reinterpret_cast<const double2 *>(m.taucmcl + base + 2 * h);
                        const double2 c = *reinterpret_cast<const double2 *>(m.ciwpmcl + base + 2 * h);
                        const double2 d = *reinterpret_cast<const double2 *>(m.clwpmcl + base + 2 * h);
                        cf[2 * h] = a.x; cf[2 * h + 1] = a.y; tau[2 * h] = b.x; tau[2 * h + 1] = b.y;
                        ci[2 * h] = c.x; ci[2 * h + 1] = c.y; cw[2 * h] = d.x; cw[2 * h + 1] = d.y;
                    } else {
                        cf[2 * h] = cf[2 * h + 1] = 0.0; tau[2 * h] = tau[2 * h + 1] = 0.0;
                        ci[2 * h] = ci[2 * h + 1] = 0.0; cw[2 * h] = cw[2 * h + 1] = 0.0;
                    }
                }
            }
            double od[4];
            float ocf[4], oef[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                double t = tau[j];
                if (cf[j] >= cldmin && (ci[j] + cw[j] >= cldmin || t >= cldmin)) {        // cldprmc :181-183
                    if (inflag == 1) err = E_MC_INFLAG1;                                     // :190-191
                    else if (inflag == 2) {
                        double a_i = 0.0, a_l = 0.0;
                        if (ci[j] != 0.0 && iceflag >= 0 && iceflag <= 3) { a_i = ai; if (ice_err && !err) err = ice_err; }      // the first stop in the reference's order
                        if (cw[j] != 0.0) {
                            if (liqflag == 0) a_l = al;
                            else if (liqflag == 1) { a_l = al; if (liq_err && !err) err = liq_err; }       // (ice is checked first: cldprmc :204-254)
                        }
                        t = ci[j] * a_i + cw[j] * a_l;                                          // :267-268
                    }
                }
                od[j] = 0.0; oef[j] = 0.f;
                if (cf[j] == 1.0) {                                                             // rtrnmc :311-317
                    od[j] = secdiff * t;
                    oef[j] = (float)((1. - exp(-od[j])) * cf[j]);
                    any = 1;
                }
                ocf[j] = (float)cf[j];
            }
            const size_t so = ((size_t)quad * nlay + (lay - 1)) * ncb + col;
            double2 *po = reinterpret_cast<double2 *>(W.odg + so * 4);
            po[0] = make_double2(od[0], od[1]);
            po[1] = make_double2(od[2], od[3]);
            float4 *pf = reinterpret_cast<float4 *>(W.cfef + so * 8);
            pf[0] = make_float4(ocf[0], ocf[1], ocf[2], ocf[3]);
            pf[1] = make_float4(oef[0], oef[1], oef[2], oef[3]);
        }
    }
    W.cflag[(size_t)lay * ncb + col] = any;
    if (any) atomicOr(&W.cflag[col], 8);
    if (any && lay > *reinterpret_cast<volatile int *>(&W.btop[col >> 6])) atomicMax(&W.btop[col >> 6], lay);
    if (any && lay < *reinterpret_cast<volatile int *>(&W.bbot[col >> 6])) atomicMin(&W.bbot[col >> 6], lay);
    if (lay == 1) W.cflag[(size_t)(nlay + 1) * ncb + col] = 0;
    if (err) atomicCAS(W.err, 0, err);
}

// ------------------------------------------------------------------------------------------------
// McICA sub-column generator: mcica_subcol_lw / generate_stochastic_clouds (src/mcica_subcol_gen_lw.f90:183-703).
// The GCM routine does not compile as shipped; the per-column semantics are those of its
// compilable one-column statement, src/mcica_subcol_gen_lw.1col.f90:171-710.
//   k_subcol_kiss  irng = 0: every column owns a KISS stream seeded from its four lowest layer pressures
//                  (:460-474) and consumed in (sub-column, layer) order -> a thread per (column, 8 sub-columns), each
//                  sub-column's stream reached by jump-ahead; the decisions leave as bytes of the bit mask.
//   k_subcol_slab  irng = 1: the Mersenne-Twister stream is ONE sequence over (sub-column, column, layer)
//                  (:497-503); k_mt_jump / k_mt_fill draw it chunk-parallel and this kernel applies the overlap rules to
//                  the slab of one sub-column.
//   k_subcol_expand  mask -> the (140,ncol,nlay) arrays of the reference interface (:664-680).
//   k_alpha        get_alpha (src/mcica_subcol_gen_lw.f90:68-180).
// Integer arithmetic is 32-bit wrap-around with logical shifts and the uniform deviates are formed without
// FMA contraction, so the cloud masks are bit-identical to the reference's.
// ------------------------------------------------------------------------------------------------
struct SubcolIn { const double *play, *cldfrac, *alpha; };      // each (ncol_total, nlay), device pointers

struct Kiss { unsigned a, b, c, d; };

// multiplier x (low half of s) + (high half of s): one v_mad_u32_u16, which reads the low halves of its factors (the compiler
// masks the half out first and multiplies with v_mad_u32_u24)
__device__ __forceinline__ unsigned kiss_mwc(unsigned s, unsigned mul)
{
    unsigned r;
    const unsigned carry = s >> 16;
    asm("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(r) : "v"(s), "s"(mul), "v"(carry));
    return r;
}
// 69069 a + 1327217885 (mod 2^32) from 24-bit multiplies, which run at full rate where the 32-bit v_mul_lo_u32 takes four issue
// slots: 69069 x (low 24 bits of a) + the constant, plus (0xCD = 69069 mod 256) x (top byte of a) shifted to the top byte
__device__ __forceinline__ unsigned kiss_lcg(unsigned a)
{
    unsigned h;
    const unsigned top = a >> 24;
    asm("v_mul_u32_u24_e32 %0, 0xcd, %1" : "=v"(h) : "v"(top));
    return (h << 24) + (__umul24(a, 69069u) + 1327217885u);
}
__device__ __forceinline__ void kiss_step(Kiss &s)             // kissvec's state advance, src/mcica_subcol_gen_lw.f90:711-745
{
    s.a = kiss_lcg(s.a);
    s.b ^= s.b << 13; s.b ^= s.b >> 17; s.b ^= s.b << 5;
    s.c = kiss_mwc(s.c, 18000u);
    s.d = kiss_mwc(s.d, 30903u);
}
__device__ __forceinline__ int kiss_int(Kiss &s)               // ... the integer it returns
{
    kiss_step(s);
    return (int)(s.a + s.b + (s.c << 16) + s.d);
}
__device__ __forceinline__ double kiss_unit(int k)             // ... and the deviate the reference forms from it
{
#pragma clang fp contract(off)
    const double r = (double)k * 2.328306e-10;
    return r + 0.5;
}
__device__ __forceinline__ double kiss_next(Kiss &s) { return kiss_unit(kiss_int(s)); }

// kiss_unit is strictly increasing in k (one step of k is 2.3e-10, an ulp of the sum at most 1.1e-16), so a comparison of a deviate
// with a value v that does not depend on other deviates is a comparison of the integers: kiss_unit(k) >= v  <=>  k >= T(v) with
// T(v) the smallest such k.  T = INT_MIN when every k qualifies, INT_MAX + 1 when none does (v = NaN included).
__device__ __forceinline__ long long kiss_threshold(double v)
{
#pragma clang fp contract(off)
    constexpr long long LO = -2147483648ll, HI = 2147483647ll;
    if (!(kiss_unit((int)HI) >= v)) return HI + 1;
    if (kiss_unit((int)LO) >= v) return LO;
    double g = (v - 0.5) / 2.328306e-10;                        // within a step or two of the answer, which lies in (LO, HI]
    g = g < -2147483647. ? -2147483647. : (g > 2147483647. ? 2147483647. : g);
    long long t = (long long)g;
    for (int it = 0; it < 64 && t > LO + 1 && kiss_unit((int)(t - 1)) >= v; it++) t--;
    for (int it = 0; it < 64 && t < HI && !(kiss_unit((int)t) >= v); it++) t++;
    return t;
}

// Jump-ahead of the stream by n draws.  The four component generators are each a linear map of their own state:
//   a  (congruential, mod 2^32)      a -> A a + B with (A, B) the n-fold composition;
//   b  (xorshift 13/17/5)            linear over GF(2): the images X[i] of the 32 unit vectors under n steps;
//   c, d (multiply-with-carry, multipliers 18000 / 30903, base 2^16)   the 32-bit word s = carry 2^16 + value satisfies
//        2^16 s' = s (mod m), m = multiplier 2^16 - 1, i.e. s' = multiplier s (mod m).  Two real steps bring any 32-bit word into
//        [0, m]; 0 and m are fixed points and every other word stays in [1, m-1], where the residue names the word.  So n >= 2 steps
//        are two steps and a multiplication by P = multiplier^(n-2) mod m.
// The host fills the constants (kissjump.hpp, kiss_jump_entry).
// (struct KissJump and the moduli KISS_MC / KISS_MD: kissjump.hpp)

template <unsigned M>
__device__ __forceinline__ unsigned kiss_mwc_mul(unsigned s, unsigned P)
{
    const unsigned r = (unsigned)(((unsigned long long)s * (unsigned long long)P) % (unsigned long long)M);
    return s == M ? M : r;
}
__device__ __forceinline__ void kiss_jump(Kiss &s, const KissJump &J)
{
    if (J.n < 2u) { if (J.n == 1u) kiss_step(s); return; }
    s.a = J.A * s.a + J.B;
    unsigned b = 0u;
#pragma unroll
    for (int i = 0; i < 32; i++) b ^= (0u - ((s.b >> i) & 1u)) & J.X[i];
    s.b = b;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        s.c = 18000u * (s.c & 65535u) + (s.c >> 16);
        s.d = 30903u * (s.d & 65535u) + (s.d >> 16);
    }
    s.c = kiss_mwc_mul<KISS_MC>(s.c, J.Pc);
    s.d = kiss_mwc_mul<KISS_MD>(s.d, J.Pd);
}

// overlap rule applied to the deviate of (sub-column, layer l) given the final deviate of layer l-1
__device__ __forceinline__ double overlap_rule(int icld, int l, double x, double x2, double prev, double cf_below, double alpha_l)
{
#pragma clang fp contract(off)
    if (l > 0) {
        if (icld == 2) {                                        // maximum-random, .1col :440-448
            const double one_m = 1. - cf_below;
            if (prev > one_m) x = prev;
            else x = x * one_m;
        } else if (icld == 4 || icld == 5) {                    // exponential(-random), .1col :492-496, :521-525
            if (x2 < alpha_l) x = prev;
        }
    }
    return x;
}

// k_subcol_kiss: a work-group is KJ_COLS columns x all sub-columns; a thread owns 8 consecutive sub-columns of one column (one byte
// of the mask) and walks the layers once, with the eight streams side by side: each was brought to its place in the column's stream
// by jump-ahead (the reference draws sub-column after sub-column, layer after layer - :475-530 - so sub-column s starts
// permuteseed + s x (draws per sub-column) draws into the stream).  What a decision is compared with depends on (column, layer)
// only: the work-group forms those values once, into LDS, as integer thresholds where the rule allows it (random, maximum,
// exponential: 1, 3, 4/5) and as 1 - cldfrac for the maximum-random rule, whose deviates are rescaled in floating point.
// Lanes 4 c .. 4 c + 3 of a wave hold the four bytes of one column's mask word and neighbouring columns follow, so one byte
// store per layer writes 64 contiguous bytes.  (The first version - a thread per column walking its 140 x nlay decisions in stream
// order with cldfrac / alpha re-read for every sub-column - moved 161 GB per 1e6 columns through HBM: 73 KB per wave of re-read
// working set, sixteen waves a CU, against 128 KB of L2 a CU.)
constexpr int KJ_COLS = 16;
constexpr int KJ_NWORD = MASK_WORDS;                 // mask words of a column = waves of a work-group
constexpr int KJ_BLOCK = 64 * KJ_NWORD;
constexpr int KJ_NGROUP = 4 * KJ_NWORD;             // 8-sub-column groups, the last ones possibly short or empty

// RULE 1 random, 2 maximum-random, 3 maximum, 4 exponential / exponential-random (icld 4 and 5 differ in alpha only).
// jt[g]: jump from the seed to the first sub-column of group g; jsub: jump by one sub-column.
// (waves per SIMD pinned to what the kernel needs without spilling: left to itself the allocator took 79 / 97 / 95 registers for rules
// 1 / 2 / 4 after an unrelated change of the argument struct - four waves instead of six, 3.7 -> 4.5 ms per 1e6 columns)
__host__ __device__ constexpr int kiss_waves(int rule) { return rule == 3 ? 5 : 6; }
template <int RULE>
__global__ __launch_bounds__(KJ_BLOCK, kiss_waves(RULE)) void k_subcol_kiss(Workspace W, SubcolIn in, const KissJump *jt, KissJump jsub, int ncol, int col0, int nb, int nlay)
{
#pragma clang fp contract(off)
    extern __shared__ int4 kj_thr[];                             // [nlay][KJ_COLS]
    __shared__ int kj_top;                                       // highest layer with cloud in any of the work-group's columns
    const int tid = threadIdx.x;
    if (tid == 0) kj_top = -1;
    __syncthreads();
    int top = -1;
    const int cl = (tid >> 2) & (KJ_COLS - 1);
    const int g = (tid >> 6) * 4 + (tid & 3);                    // sub-columns 8 g .. 8 g + 7 = byte g & 3 of mask word g >> 2
    const int cb = blockIdx.x * KJ_COLS;
    const double cldmin = 1.0e-20;
    // pass 1: the highest layer with cloud in any of the work-group's columns.  Every sub-column's stream is positioned on its own, so
    // nothing depends on the draws of the layers above it: no deviate reaches 1 - 0 there, the walk ends at `ltop` (the stratosphere
    // of every column, most of the troposphere of many) and thresholds are formed up to it only.
    for (int e = tid; e < nlay * KJ_COLS; e += KJ_BLOCK) {
        const int c = e & (KJ_COLS - 1), l = e / KJ_COLS;
        if (cb + c < nb && in.cldfrac[(size_t)col0 + (size_t)(cb + c) + (size_t)ncol * l] >= cldmin) top = l;       // (e ascends with l)
    }
    if (top >= 0) atomicMax(&kj_top, top);
    __syncthreads();
    const int ltop = kj_top;
    for (int e = tid; e < (ltop + 1) * KJ_COLS; e += KJ_BLOCK) {
        const int c = e & (KJ_COLS - 1), l = e / KJ_COLS;
        int4 t = make_int4(0, (int)0x80000000, 0, 0);
        if (cb + c < nb) {
            const size_t cell = (size_t)col0 + (size_t)(cb + c) + (size_t)ncol * l;
            double cf = in.cldfrac[cell];
            if (cf < cldmin) cf = 0.0;
            const double v = 1. - cf;                            // cloudy: deviate >= v (:655-661)
            if (RULE == 2) {
                t.x = __double2loint(v); t.y = __double2hiint(v);
            } else {
                const long long T = kiss_threshold(v);
                t.x = T > 2147483647ll ? 2147483647 : (int)T;
                t.w = T > 2147483647ll ? 0 : 0xff;               // no integer reaches v: the byte is cleared after the compare
                if (RULE == 4 && l > 0) {                        // deviate2 < alpha keeps the deviate of the layer below (:492-496)
                    const double al = in.alpha[cell];
                    const long long Ta = al != al ? -2147483648ll : kiss_threshold(al);
                    t.y = Ta > 2147483647ll ? 2147483647 : (int)Ta;
                    t.z = Ta > 2147483647ll ? 1 : 0;             // every integer is below alpha
                }
            }
        }
        kj_thr[e] = t;
    }
    __syncthreads();
    if (cb + cl >= nb) return;
    const size_t gc = (size_t)col0 + (size_t)(cb + cl);
    Kiss s[8];
    {
        const double p1 = in.play[gc] * 1.e2, p2 = in.play[gc + (size_t)ncol] * 1.e2;
        const double p3 = in.play[gc + (size_t)ncol * 2] * 1.e2, p4 = in.play[gc + (size_t)ncol * 3] * 1.e2;
        if (p1 < p2) { atomicCAS(W.err, 0, (int)E_KISS_PMID); return; }            // :463-466
        s[0].a = (unsigned)(int)((p1 - (double)(long long)p1) * 1000000000.);
        s[0].b = (unsigned)(int)((p2 - (double)(long long)p2) * 1000000000.);
        s[0].c = (unsigned)(int)((p3 - (double)(long long)p3) * 1000000000.);
        s[0].d = (unsigned)(int)((p4 - (double)(long long)p4) * 1000000000.);
    }
    // sub-columns past NGPT in the last word: their streams run along (no divergence in the loop below), their bits are cleared
    const int nv = min(8, max(0, NGPT - 8 * g));
    const unsigned live = (1u << nv) - 1u;
    unsigned char *out = reinterpret_cast<unsigned char *>(W.mask + ((size_t)(g >> 2) * nlay) * W.mask_stride + gc) + (g & 3);
    const size_t ostep = W.mask_stride * sizeof(unsigned);
    if (ltop < 0) {                                              // sixteen cloud-free columns
        for (int l = 0; l < nlay; l++) out[(size_t)l * ostep] = (unsigned char)0;
        return;
    }
    kiss_jump(s[0], jt[g]);
#pragma unroll
    for (int j = 1; j < 8; j++) { s[j] = s[j - 1]; kiss_jump(s[j], jsub); }
    int kx[8];
    double px[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { kx[j] = RULE == 3 ? kiss_int(s[j]) : 0; px[j] = 0.0; }
    double one_m = 1.0;
    int4 t = kj_thr[cl];
#pragma unroll 1
    for (int l = 0; l <= ltop; l++) {
        const int4 tn = kj_thr[min(l + 1, ltop) * KJ_COLS + cl];
        unsigned bits = 0u;
        if (RULE == 2) {                                         // maximum-random, .1col :440-448
            const double v = __hiloint2double(t.y, t.x);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                double x = kiss_next(s[j]);
                if (l > 0) x = px[j] > one_m ? px[j] : x * one_m;
                px[j] = x;
                bits |= x >= v ? 1u << j : 0u;
            }
            one_m = v;
        } else {
            const bool below = t.z != 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (RULE == 1) kx[j] = kiss_int(s[j]);
                if (RULE == 4) {
                    const int k = kiss_int(s[j]), k2 = kiss_int(s[j]);
                    kx[j] = ((k2 < t.y) | below) ? kx[j] : k;
                }
                bits |= kx[j] >= t.x ? 1u << j : 0u;
            }
            bits &= (unsigned)t.w;
        }
        out[(size_t)l * ostep] = (unsigned char)(bits & live);
        t = tn;
    }
    for (int l = ltop + 1; l < nlay; l++) out[(size_t)l * ostep] = (unsigned char)0;
}

// ---- Mersenne Twister on the device (irng = 1) ----------------------------------------------------------------------------------
// The stream is ONE MT19937 sequence over (sub-column, column, layer) (src/mcica_subcol_gen_lw.f90:497-503).  It is cut into chunks,
// the state at the start of every chunk is reached by jump-ahead (k_mt_jump applies g(x) = x^n mod phi(x) to a state by Horner's
// scheme; mtjump.hpp builds the polynomials and has the references), and k_mt_fill regenerates each chunk's deviates from its state.
// A state is 624 words in canonical order: st[0] = x_k (only its top bit matters) ... st[623] = x_{k+623}; deviate number t of the
// stream is the tempered x_{t+624}.
constexpr int MT_NW = 624, MT_BLOCK = 64, MT_PW = 312, MT_R = (MT_NW + 63) / 64;
// (One wavefront per state: with ten waves the two barriers around every XOR pass of k_mt_jump cost 11 ms per round of 19 937 steps and
// the four per block of k_mt_fill 1 us; a single wave needs no barrier beyond its own LDS ordering - 2 ms and 0.25 us.)

__device__ __forceinline__ unsigned mt_next(unsigned x0, unsigned x1, unsigned x397)
{
    const unsigned y = (x0 & 0x80000000u) | (x1 & 0x7fffffffu);
    return x397 ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// dst state = g(A) src state.  Work-group (x, y): src = st[src0 + y ystride + x xstride], dst = src + doff.
// Horner's scheme acc <- A acc ^ g_i s, taken 64 coefficients at a time (A is linear):
//      acc <- A^64 acc  ^  sum_{t=0..63} g_{i-t} A^(63-t) s.
// A^64 on a state is 64 new words, each a function of old words only (64 < 227): one word per lane.  A^m s is the window m .. m+623 of
// the source's own word sequence, so the sum is, for every word j, an XOR of ext[j + 63 - t] over the set coefficients - reads of a
// static LDS array, with the ring `acc` (logical word j at (h + j) mod 624) touched once per 64 coefficients.  (Coefficient by
// coefficient, with a barrier pair around every XOR pass, a round of jumps took 12 ms; this form 0.2 ms.)
__global__ __launch_bounds__(MT_BLOCK) void k_mt_jump(unsigned *st, const unsigned long long *g, int src0, int xstride, int ystride, int doff)
{
    __shared__ unsigned acc[MT_NW], ext[MT_NW + 64 + 16];
    __shared__ unsigned long long gs[MT_PW];
    const int tid = threadIdx.x;
    const size_t si = (size_t)src0 + (size_t)blockIdx.y * ystride + (size_t)blockIdx.x * xstride;
    const unsigned *sp = st + si * MT_NW;
    unsigned *dp = st + (si + (size_t)doff) * MT_NW;
#pragma unroll
    for (int r = 0; r < MT_R; r++) {
        const int j = tid + 64 * r;
        if (j < MT_NW) { ext[j] = sp[j]; acc[j] = 0u; }
    }
    for (int j = tid; j < MT_PW; j += 64) gs[j] = g[j];
    __syncthreads();
    ext[MT_NW + tid] = mt_next(ext[tid], ext[tid + 1], ext[tid + 397]);       // words 624 .. 687 of the source's sequence
    __syncthreads();
    // the XOR pass: lane `tid` owns the ten consecutive words 10 tid .. 10 tid + 9 (lane 62 four, lane 63 none).  Going through the 64
    // coefficients from offset 63 down, the window ext[j0 + b .. j0 + b + 9] slides by one word per coefficient: one LDS read each,
    // kept in a ring of ten registers whose slot numbers are compile-time constants in the unrolled loop.
    const int j0 = 10 * tid;
    const int nk = tid < 62 ? 10 : (tid == 62 ? 4 : 0);
    int h = 0;
    bool zero = true;                                                         // acc is still all zero (leading zero coefficients)
    for (int w = MT_PW - 1; w >= 0; w--) {
        const unsigned long long mv = gs[w];                                  // coefficients 64 w + 63 (offset 63) ... 64 w (offset 0)
        const unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)mv), mhi = __builtin_amdgcn_readfirstlane((unsigned)(mv >> 32));
        if (zero && (mlo | mhi) == 0u) continue;
        if (!zero) {                                                          // acc <- A^64 acc
            const int p0 = h + tid < MT_NW ? h + tid : h + tid - MT_NW;
            const int p1 = p0 + 1 < MT_NW ? p0 + 1 : 0;
            const int p397 = p0 + 397 < MT_NW ? p0 + 397 : p0 + 397 - MT_NW;
            const unsigned nw = mt_next(acc[p0], acc[p1], acc[p397]);
            __syncthreads();
            acc[p0] = nw;                                                     // the 64 oldest words make room for the 64 newest
            h = h + 64 < MT_NW ? h + 64 : h + 64 - MT_NW;
            __syncthreads();
        }
        if ((mlo | mhi) != 0u) {
            unsigned v[10], P[10];
#pragma unroll
            for (int k = 0; k < 10; k++) { v[k] = 0u; P[(63 + k) % 10] = ext[j0 + 63 + k]; }
#pragma unroll
            for (int b = 63; b >= 0; b--) {
                const bool on = b >= 32 ? ((mhi >> (b - 32)) & 1u) != 0u : ((mlo >> b) & 1u) != 0u;       // (uniform)
                if (on) {
#pragma unroll
                    for (int k = 0; k < 10; k++) v[k] ^= P[(b + k) % 10];
                }
                if (b > 0) P[(b - 1) % 10] = ext[j0 + b - 1];                 // replaces word j0 + b + 9, which has the same slot
            }
#pragma unroll
            for (int k = 0; k < 10; k++) {
                if (k < nk) { const int j = j0 + k; const int p = h + j < MT_NW ? h + j : h + j - MT_NW; acc[p] ^= v[k]; }
            }
            zero = false;
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < MT_R; r++) {
        const int j = tid + 64 * r;
        if (j < MT_NW) { const int p = h + j < MT_NW ? h + j : h + j - MT_NW; dp[j] = acc[p]; }
    }
}

// Deviates of chunk blockIdx.x of slab blockIdx.y: rnd[y per + m C .. y per + min((m+1) C, per)) from the state st[state0 + y M + m].  A block of 624 new words
// depends on the previous 624 in three waves of the recurrence (i < 227 on old words only, 227 <= i < 454 on the first wave's words,
// the rest on the second's; word 623 needs the new word 0).  genrand_real1: tempered word / (2^32 - 1) (src/mcica_random_numbers.f90:262-295).
__global__ __launch_bounds__(MT_BLOCK) void k_mt_fill(const unsigned *st, double *rnd, int state0, int M, unsigned long long C, unsigned long long per)
{
#pragma clang fp contract(off)
    __shared__ unsigned a[MT_NW], b[MT_NW];
    const int tid = threadIdx.x;
    const unsigned long long lo = (unsigned long long)blockIdx.x * C;
    if (lo >= per) return;
    const unsigned long long len = (per - lo < C) ? per - lo : C;
    rnd += (size_t)blockIdx.y * per;                             // slab blockIdx.y of this launch: states state0 + y M ...
    for (int j = tid; j < MT_NW; j += 64) a[j] = st[((size_t)state0 + (size_t)blockIdx.y * M + blockIdx.x) * MT_NW + j];
    __syncthreads();
    unsigned *o = a, *n = b;
    for (unsigned long long base = 0; base < len; base += MT_NW) {
#pragma unroll
        for (int r = 0; r < 4; r++) { const int i = tid + 64 * r; if (i < 227) n[i] = mt_next(o[i], o[i + 1], o[i + 397]); }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) { const int i = 227 + tid + 64 * r; if (i < 454) n[i] = mt_next(o[i], o[i + 1], n[i - 227]); }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 3; r++) { const int i = 454 + tid + 64 * r; if (i < 623) n[i] = mt_next(o[i], o[i + 1], n[i - 227]); }
        if (tid == 0) n[623] = mt_next(o[623], n[0], n[396]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < MT_R; r++) {
            const int i = tid + 64 * r;
            if (i < MT_NW && base + i < len) {
                unsigned y = n[i];
                y ^= y >> 11;
                y ^= (y << 7) & 0x9d2c5680u;
                y ^= (y << 15) & 0xefc60000u;
                y ^= y >> 18;
                rnd[lo + base + i] = (double)y / 4294967295.0;
            }
        }
        unsigned *t = o; o = n; n = t;
    }
}

// rnd: the deviates of sub-column `isub` for all columns in stream order: icld == 3: [ncol]; otherwise
// [ncol][nlay][nd] with nd = 2 for icld 4/5 (CDF, CDF2), else 1.  The mask must have been zeroed.
constexpr int SLAB_GROUP = 8;       // slabs a thread takes through a chunk of layers on one load of cldfrac / alpha
__global__ __launch_bounds__(256) void k_subcol_slab(Workspace W, SubcolIn in, const double *rnd, int ncol, int nlay, int icld, int isub0, int nslab,
                                                     unsigned long long per)
{
#pragma clang fp contract(off)
    const size_t gc = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gc >= (size_t)ncol) return;
    // several slabs per launch: the bits of a mask word come from different work-groups, hence the atomic OR
    const int s0 = blockIdx.y * SLAB_GROUP, ns = min(SLAB_GROUP, nslab - s0);
    rnd += (size_t)s0 * per;
    const double cldmin = 1.0e-20;
    const bool two = icld == 4 || icld == 5;
    const int nd = two ? 2 : 1;
    double prev[SLAB_GROUP], r3[SLAB_GROUP];
#pragma unroll
    for (int j = 0; j < SLAB_GROUP; j++) { prev[j] = 0.0; r3[j] = (icld == 3 && j < ns) ? rnd[(size_t)j * per + gc] : 0.0; }
    double cf_below = 0.0;
    // layers in chunks of 8: cloud fractions and overlap parameters are requested once for the group's slabs, each slab's deviates of the
    // chunk (contiguous per column in stream order) together, then the eight dependent steps run from registers
#pragma unroll 1
    for (int l0 = 0; l0 < nlay; l0 += 8) {
        double cfc[8], alc[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int l = l0 + i < nlay ? l0 + i : nlay - 1;
            double cf = in.cldfrac[gc + (size_t)ncol * l];
            cfc[i] = cf < cldmin ? 0.0 : cf;
            alc[i] = two ? in.alpha[gc + (size_t)ncol * l] : 0.0;
        }
#pragma unroll 1
        for (int j = 0; j < ns; j++) {
            const double *rj = rnd + (size_t)j * per;
            double xs[8], x2s[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int l = l0 + i < nlay ? l0 + i : nlay - 1;
                const size_t o = (gc * nlay + l) * nd;
                xs[i] = icld == 3 ? 0.0 : rj[o];
                x2s[i] = two ? rj[o + 1] : 0.0;
            }
            const int isub = isub0 + s0 + j;
            const int w = isub >> 5;
            const unsigned bit = 1u << (isub & 31);
            double pv = 0.0, r3j = 0.0;
#pragma unroll
            for (int jj = 0; jj < SLAB_GROUP; jj++) if (jj == j) { pv = prev[jj]; r3j = r3[jj]; }
            double below = cf_below;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int l = l0 + i;
                if (l < nlay) {
                    const double x = overlap_rule(icld, l, icld == 3 ? r3j : xs[i], x2s[i], pv, below, alc[i]);
                    pv = x; below = cfc[i];
                    if (x >= 1. - cfc[i]) atomicOr(&W.mask[((size_t)w * nlay + l) * W.mask_stride + gc], bit);
                }
            }
#pragma unroll
            for (int jj = 0; jj < SLAB_GROUP; jj++) if (jj == j) prev[jj] = pv;
        }
        cf_below = cfc[7];                                    // (a short last chunk ends the loop)
    }
}

__device__ __forceinline__ int g_band(int ig)            // 1-based band of 0-based g-point ig (ngb)
{
    int b = 1;
#pragma unroll
    for (int B = 2; B <= NBND; B++) b += (ig >= band_g0(B)) ? 1 : 0;
    return b;
}

// one thread per (sub-column, column) of one layer: fully coalesced stores into the (140,ncol,nlay) arrays.
// Layers l0 .. l0 + gridDim.y - 1 are written to the output arrays starting at their layer 0.
__global__ __launch_bounds__(256) void k_subcol_expand(Workspace W, const double *ciwp, const double *clwp, const double *tauc,
                                                       int ncol, int nlay, int l0, double *cldfmcl, double *ciwpmcl, double *clwpmcl, double *taucmcl)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)NGPT * ncol) return;
    const int l = l0 + blockIdx.y;
    const int isub = (int)(e % NGPT);
    const size_t gc = e / NGPT;
    const unsigned word = W.mask[((size_t)(isub >> 5) * nlay + l) * W.mask_stride + gc];
    const bool on = (word >> (isub & 31)) & 1u;
    const size_t cl = gc + (size_t)ncol * l;
    const size_t o = e + (size_t)NGPT * ncol * blockIdx.y;
    cldfmcl[o] = on ? 1.0 : 0.0;
    ciwpmcl[o] = on ? ciwp[cl] : 0.0;
    clwpmcl[o] = on ? clwp[cl] : 0.0;
    taucmcl[o] = on ? tauc[(g_band(isub) - 1) + (size_t)NBND * cl] : 0.0;
}

// 1 / decorrelation length of a column (idcor = 1: from its latitude and the day of the year, :140-152) and the layer's alpha from it
__device__ __forceinline__ double alpha_decorr_inv(int idcor, double decorr_con, double lat, int juldat)
{
    const double am1 = 1.4315, am2 = 2.1219, am4 = -25.584, amr = 7.0;
    double decorr_len, decorr_inv = 1.0;
    if (idcor == 1) {                               // latitude / day-of-year dependent decorrelation length, :140-152
        double am3;
        if (juldat > 181) am3 = -4. * amr / 365. * (juldat - 272);
        else am3 = 4. * amr / 365. * (juldat - 91);
        const double y = lat - am3;
        decorr_len = (am1 + am2 * exp(-(y * y) / (am4 * am4))) * 1.e3;
    } else {
        decorr_len = decorr_con;
    }
    if (decorr_len >= 0.0) decorr_inv = 1.0 / decorr_len;
    return decorr_inv;
}
// (dz, cf: the layer's; dzm, cfm: those of the layer below it)
__device__ __forceinline__ double alpha_of(int icld, double decorr_inv, double dz, double dzm, double cf, double cfm)
{
    double a = exp(-(0.5 * (dz + dzm)) * decorr_inv);
    if (icld == 5 && cf == 0.0 && cfm > 0.0) a = 0.0;
    return a;
}
__global__ __launch_bounds__(256) void k_alpha(int ncol, int nlay, int icld, int idcor, double decorr_con, const double *dz,
                                               const double *lat, int juldat, const double *cldfrac, double *alpha)
{
    const size_t gc = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gc >= (size_t)ncol) return;
    const int k = blockIdx.y;                       // layer index 0 .. nlay-1
    if (!(icld == 4 || icld == 5)) return;
    const double decorr_inv = alpha_decorr_inv(idcor, decorr_con, idcor == 1 ? lat[gc] : 0.0, juldat);
    const size_t o = gc + (size_t)ncol * k;
    double a = 0.0;
    if (k > 0) {
        const size_t om = o - (size_t)ncol;
        a = alpha_of(icld, decorr_inv, dz[o], dz[om], cldfrac[o], cldfrac[om]);
    }
    alpha[o] = a;
}
// ... on DEVICE arrays in the caller's own form and width (rrtmg_lw_hip_get_alpha_device_view): R the element type, ld the columns
// between two rows of a column-fastest array, layer_fastest / top_first as rrtmg_lw_hip_array_form states them.  The value of reference
// layer k goes where the form stores layer k; the layer below it, k - 1, is the NEXT index of a top-first array.  lat is per column.
template <class R>
__global__ __launch_bounds__(256) void k_alpha_view(int ncol, int nlay, size_t ld, int layer_fastest, int top_first, int icld, int idcor, double decorr_con,
                                                    const R *dz, const R *lat, int juldat, const R *cldfrac, R *alpha)
{
    const size_t gc = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gc >= (size_t)ncol) return;
    const int k = blockIdx.y;                       // reference layer index 0 .. nlay-1, 0 at the surface
    const double decorr_inv = alpha_decorr_inv(idcor, decorr_con, idcor == 1 ? (double)lat[gc] : 0.0, juldat);
    const auto at = [&](int kr) -> size_t {
        const size_t kk = (size_t)(top_first ? nlay - 1 - kr : kr);
        return layer_fastest ? gc * (size_t)nlay + kk : gc + ld * kk;
    };
    const size_t o = at(k);
    double a = 0.0;
    if (k > 0) {
        const size_t om = at(k - 1);
        a = alpha_of(icld, decorr_inv, (double)dz[o], (double)dz[om], (double)cldfrac[o], (double)cldfrac[om]);
    }
    alpha[o] = (R)a;
}

// ------------------------------------------------------------------------------------------------
// k_cloudcover : rrtmg_lw_hip_mcica_cloud_cover* - what the sub-columns of W.mask (one sample) realise of the cloud field, counted, not
//               estimated: per (column, layer) the sub-columns that are cloudy in the layer (cldlay) and in the layer or any above it
//               (cldcum; its value at the surface layer is the total cover, cldtot), and the mask itself with the bits past NGPT cleared
//               (submask).  Lanes are consecutive columns - for a fixed (word, layer) their mask words are consecutive, and so are the
//               values of a row of a column-fastest output -; a thread walks its column from the top layer down with the MASK_WORDS
//               running OR words in registers.  Outputs in the caller's form (R: element type; ld, layer_fastest, top_first as
//               rrtmg_lw_hip_array_view states them: the count of reference layer k goes where the form keeps layer k), each optional.
//               Several samples: sample 0 stores its counts (first), the others add theirs to what the arrays hold, the last one also
//               divides (last) - counts are at most 256 x 64 and exact in float32 too; every value leaves as ONE float64 division
//               count / denom, rounded to R.  cloud = 0 (icld = 0): no mask is read, every count is zero.
// ------------------------------------------------------------------------------------------------
struct CoverArgs {
    void *cldtot, *cldcum, *cldlay;     // (ncol), (ncol,nlay), (ncol,nlay) of R, or null
    unsigned *submask;                  // (ncol,nlay,MASK_WORDS): column-fastest rows ld apart, or C order with layer_fastest; or null
    unsigned long long ncol, ld;
    int nlay, layer_fastest, top_first;
    int cloud, first, last;
    double denom;                       // NGPT x samples
};
template <class R>
__device__ __forceinline__ void cover_put(void *p, size_t at, int count, const CoverArgs &a)
{
    if (!p) return;
    R *const q = static_cast<R *>(p) + at;
    double v = (double)count;
    if (!a.first) v += (double)*q;
    if (a.last) v = v / a.denom;
    *q = (R)v;
}
template <class R>
__global__ __launch_bounds__(256) void k_cloudcover(Workspace W, CoverArgs a)
{
    const size_t gc = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gc >= (size_t)a.ncol) return;
    const int nlay = a.nlay;
    unsigned seen[MASK_WORDS] = {};
    int ccum = 0;
    for (int l = nlay - 1; l >= 0; l--) {
        const size_t kk = (size_t)(a.top_first ? nlay - 1 - l : l);
        int clay = 0;
        ccum = 0;
#pragma unroll
        for (int w = 0; w < MASK_WORDS; w++) {
            unsigned m = a.cloud ? W.mask[((size_t)w * nlay + l) * W.mask_stride + W.mask_col0 + gc] : 0u;
            if (w == MASK_WORDS - 1 && (NGPT & 31)) m &= (1u << (NGPT & 31)) - 1u;       // (the generator may leave bits past the last sub-column)
            seen[w] |= m;
            clay += __popc(m);
            ccum += __popc(seen[w]);
            if (a.submask) a.submask[a.layer_fastest ? (gc * (size_t)nlay + kk) * MASK_WORDS + w : ((size_t)w * nlay + kk) * a.ld + gc] = m;
        }
        const size_t at = a.layer_fastest ? gc * (size_t)nlay + kk : gc + a.ld * kk;
        cover_put<R>(a.cldlay, at, clay, a);
        cover_put<R>(a.cldcum, at, ccum, a);
    }
    cover_put<R>(a.cldtot, gc, ccum, a);
}

// ------------------------------------------------------------------------------------------------
// k_cloudoptics_col / k_cloudoptics : rrtmg_lw_hip_cloud_optics* - the cloud optical depth per spectral band as cldprop (imca = 0,
//               src/rrtmg_lw_cldprop.f90:173-293, with rtrn's band -> cloud-band map, src/rrtmg_lw_rtrn.f90:343-349) or cldprmc (imca = 1,
//               src/rrtmg_lw_cldprmc.f90:173-273, on the cloudy cells the generator expands from the grid-mean inputs) forms it, BEFORE the
//               diffusivity secant, and the secants themselves (rtrn :280-288 from inatm's pwvcm).  The table logic is k_cloudlay's and
//               k_cloudmc's, restated here under contract(off): every product, sum and quotient rounds on its own, so that the values
//               are defined operation by operation (include/rrtmg_lw_hip.h); the solver's kernels are not touched.
//               Inputs are read and outputs stored in the caller's form (R: element type; ld, layer_fastest, top_first as
//               rrtmg_lw_hip_array_view states them), lanes = consecutive columns.
//   k_cloudoptics_col  one thread per column: the walk that carries cldprop's band count from layer to layer (k_cloudscan's) - the count
//               in effect at every layer and the final one go to `nbat` ([nlay + 1][ncol] bytes), the final one to ncbands -, and the
//               column sums of inatm -> pwvcm -> secdiff (k_colprep's).
//   k_cloudoptics      one thread per (column, layer): the sixteen band values of the cell.
// ------------------------------------------------------------------------------------------------
struct CloudOpticsArgs {
    const void *cldfr, *taucld, *cicewp, *cliqwp, *reice, *reliq, *plev, *h2ovmr;      // of R; the cloud six null when neither taucloud nor ncbands is asked for
    void *taucloud, *secdiff;           // (ncol,nlay,16) like tauaer, (ncol,16) like emis, of R, or null
    int *ncbands;                       // (ncol) or null
    unsigned char *nbat;                // [nlay + 1][ncol]: the band count cldprop had reached at each layer; row nlay: at the end of the column
    unsigned long long ncol, ld;
    int nlay, layer_fastest, top_first;
    int imca, inflag, iceflag, liqflag;
    int *err;
};
template <class R> __device__ __forceinline__ double co_get(const void *p, size_t at) { return (double)static_cast<const R *>(p)[at]; }
// where the form keeps element (column i, reference layer k) of a (ncol,nlay) array ...
__device__ __forceinline__ size_t co_lay(const CloudOpticsArgs &a, size_t i, int k)
{
    const size_t kk = (size_t)(a.top_first ? a.nlay - 1 - k : k);
    return a.layer_fastest ? i * (size_t)a.nlay + kk : i + a.ld * kk;
}
// ... and band b of taucld at that cell: (16,ld,nlay), or (ncol,nlay,16) in C order
__device__ __forceinline__ size_t co_tau(const CloudOpticsArgs &a, size_t i, int k, int b)
{
    const size_t kk = (size_t)(a.top_first ? a.nlay - 1 - k : k);
    return a.layer_fastest ? (i * (size_t)a.nlay + kk) * NBND + b : (size_t)b + (size_t)NBND * (i + a.ld * kk);
}
template <class R>
__device__ __forceinline__ double co_tauctot(const CloudOpticsArgs &a, size_t i, int k)      // cldprop :180-183, in band order
{
#pragma clang fp contract(off)
    double tauctot = 0.0;
    for (int ib = 0; ib < NBND; ib++) tauctot = tauctot + co_get<R>(a.taucld, co_tau(a, i, k, ib));
    return tauctot;
}

template <class R>
__global__ __launch_bounds__(256) void k_cloudoptics_col(CloudOpticsArgs a)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)a.ncol) return;
    const int nlay = a.nlay;
    if (a.nbat) {
        int ncbands = a.imca ? NBND : 1;
        if (!a.imca) {
#pragma unroll 4
            for (int k = 0; k < nlay; k++) {
                const size_t at = co_lay(a, i, k);
                const double cf = co_get<R>(a.cldfr, at), ciwp = co_get<R>(a.cicewp, at), clwp = co_get<R>(a.cliqwp, at);
                const double cwp = ciwp + clwp;
                bool enters = cf >= 1.e-20 && cwp >= 1.e-20;
                if (cf >= 1.e-20 && !enters) enters = co_tauctot<R>(a, i, k) >= 1.e-20;
                if (enters) {
                    if (a.inflag == 0 || a.inflag == 1) ncbands = 16;
                    else if (a.inflag == 2) {
                        if (ciwp != 0.0) { if (a.iceflag == 1) ncbands = 5; else if (a.iceflag == 2 || a.iceflag == 3) ncbands = 16; }
                        if (clwp != 0.0 && a.liqflag == 1) ncbands = 16;
                    }
                }
                a.nbat[(size_t)k * a.ncol + i] = (unsigned char)ncbands;
            }
        }
        a.nbat[(size_t)nlay * a.ncol + i] = (unsigned char)ncbands;
        if (a.ncbands) a.ncbands[i] = ncbands;
    }
    if (!a.secdiff) return;
    // inatm's column sums (src/rrtmg_lw_rad.nomcica.f90:795-863) and rtrn's secants (:280-288), as k_colprep forms them
    const double amd = 28.9660, amw = 18.0160, avogad = 6.02214199e+23, grav = 9.8066;
    const size_t nlev = (size_t)nlay + 1;
    const auto lev_at = [&](int k) {
        const size_t kk = (size_t)(a.top_first ? nlay - k : k);
        return a.layer_fastest ? i * nlev + kk : i + a.ld * kk;
    };
    const double pz0 = co_get<R>(a.plev, lev_at(0));
    double amttl = 0.0, wvttl = 0.0, pzlo = pz0;
#pragma unroll 8
    for (int k = 0; k < nlay; k++) {
        const double w1v = co_get<R>(a.h2ovmr, co_lay(a, i, k));
        const double pzl = co_get<R>(a.plev, lev_at(k + 1));
        const double amm = (1. - w1v) * amd + w1v * amw;
        const double coldry = (pzlo - pzl) * 1.e3 * avogad / (1.e2 * grav * amm * (1. + w1v));
        pzlo = pzl;
        const double w1 = coldry * w1v;
        amttl = amttl + coldry + w1;
        wvttl = wvttl + w1;
    }
    const double wvsh = (amw * wvttl) / (amd * amttl);
    const double pwvcm = wvsh * (1.e3 * pz0) / (1.e2 * grav);
    const double a0[16] = {1.66, 1.55, 1.58, 1.66, 1.54, 1.454, 1.89, 1.33, 1.668, 1.66, 1.66, 1.66, 1.66, 1.66, 1.66, 1.66};
    const double a1[16] = {0.00, 0.25, 0.22, 0.00, 0.13, 0.446, -0.10, 0.40, -0.006, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00};
    const double a2[16] = {0.00, -12.0, -11.7, 0.00, -0.72, -0.243, 0.19, -0.062, 0.414, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00, 0.00};
#pragma unroll
    for (int b = 0; b < NBND; b++) {
        double sd = 1.66;
        if (!(b == 0 || b == 3 || b >= 9)) {
            sd = a0[b] + a1[b] * exp(a2[b] * pwvcm);
            if (sd > 1.80) sd = 1.80;
            if (sd < 1.50) sd = 1.50;
        }
        static_cast<R *>(a.secdiff)[a.layer_fastest ? i * NBND + b : i + a.ld * b] = (R)sd;
    }
}

template <class R>
__global__ __launch_bounds__(256) void k_cloudoptics(DevTables T, CloudOpticsArgs a)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)a.ncol) return;
    const int k = blockIdx.y, nlay = a.nlay;
    const double *S = T.stat;
    const double *absice1 = S + T.sl.absice1, *absice2 = S + T.sl.absice2, *absice3 = S + T.sl.absice3, *absliq1 = S + T.sl.absliq1;
    const double cldmin = 1.e-20;
    const size_t at = co_lay(a, i, k);
    const double cf = co_get<R>(a.cldfr, at), ciwp = co_get<R>(a.cicewp, at), clwp = co_get<R>(a.cliqwp, at);
    const double cwp = ciwp + clwp;
    const int inflag = a.inflag, iceflag = a.iceflag, liqflag = a.liqflag;
    // (a band's value leaves as soon as it is formed: sixteen values indexed by a loop counter would live in scratch memory)
    const size_t kk = (size_t)(a.top_first ? nlay - 1 - k : k);
    const auto put = [&](int B, double v) {
        if (a.taucloud) static_cast<R *>(a.taucloud)[a.layer_fastest ? (i * (size_t)nlay + kk) * NBND + (B - 1) : i + a.ld * (kk + (size_t)nlay * (B - 1))] = (R)v;
    };
    int err = 0;
    bool formed = false;
    if (!a.imca) {
        // cldprop: the layer as a whole enters or does not; k_cloudlay's decisions
        bool enters = cf >= cldmin && cwp >= cldmin;
        if (cf >= cldmin && !enters) enters = co_tauctot<R>(a, i, k) >= cldmin;
        if (enters) {
            formed = true;
            const int nb_at = a.nbat[(size_t)k * a.ncol + i], ncbands = a.nbat[(size_t)nlay * a.ncol + i];
            int icemode = -1, liqmode = -1, iceind = 0, liqind = 0, index_i = 1, index_l = 1;
            double radice = 0.0, ice_single = 0.0, fint_i = 0.0, liq_single = 0.0, fint_l = 0.0;
            if (inflag == 2) {
                radice = co_get<R>(a.reice, at);
                if (ciwp == 0.0) { icemode = 0; ice_single = 0.0; iceind = 0; }
                else if (iceflag == 0) {
                    if (radice < 10.0) err = E_ICE_SMALL;
                    icemode = 0; ice_single = T.absice0[0] + T.absice0[1] / radice; iceind = 0;
                } else if (iceflag == 1) {
                    if (radice < 13.0 || radice > 130.) err = E_ICE_BOUNDS;
                    icemode = 1; iceind = 1;
                } else if (iceflag == 2) {
                    if (radice < 5.0 || radice > 131.0) err = E_ICE_BOUNDS;
                    const double factor = (radice - 2.) / 3.;
                    index_i = (int)factor; if (index_i == 43) index_i = 42;
                    fint_i = factor - (double)index_i;
                    index_i = clampi(index_i, 1, 42);           // (a size out of bounds, or NaN: the call fails or is garbage, but reads inside the table)
                    icemode = 2; iceind = 2;
                } else if (iceflag == 3) {
                    if (radice < 5.0 || radice > 140.0) err = E_ICE_GEN_BOUNDS;
                    const double factor = (radice - 2.) / 3.;
                    index_i = (int)factor; if (index_i == 46) index_i = 45;
                    fint_i = factor - (double)index_i;
                    index_i = clampi(index_i, 1, 45);
                    icemode = 3; iceind = 2;
                } else err = E_BAD_FLAG;
                if (clwp == 0.0) { liqmode = 0; liq_single = 0.0; liqind = 0; if (iceind == 1) iceind = 2; }
                else if (liqflag == 0) { liqmode = 0; liq_single = T.absliq0; liqind = 0; if (iceind == 1) iceind = 2; }
                else if (liqflag == 1) {
                    const double radliq = co_get<R>(a.reliq, at);
                    if ((radliq < 2.5 || radliq > 60.) && !err) err = E_LIQ_BOUNDS;      // (both sizes out: the reference stops at the ice check)
                    index_l = (int)(radliq - 1.5);
                    if (index_l == 0) index_l = 1;
                    if (index_l == 58) index_l = 57;
                    fint_l = radliq - 1.5 - (double)index_l;
                    index_l = clampi(index_l, 1, 57);
                    liqmode = 1; liqind = 2;
                } else err = E_BAD_FLAG;
            }
#pragma unroll 1
            for (int B = 1; B <= NBND; B++) {
                const int ib = ncbands == 1 ? 1 : (ncbands == 5 ? icb_map(B, 1) : B);      // rtrn :343-349
                double v = 0.0;
                if (ib > nb_at) v = 0.0;                                                   // (not assigned while cldprop carried fewer bands)
                else if (inflag == 0) v = co_get<R>(a.taucld, co_tau(a, i, k, ib - 1));
                else if (inflag == 1) v = T.abscld1 * cwp;
                else if (inflag == 2) {
                    int ki = icb_map(ib, iceind);
                    const int kl = icb_map(ib, liqind);
                    if (icemode == 1 && ki > 5) ki = 5;         // the stated deviation: k_cloudlay, include/rrtmg_lw_hip.h
                    double ai = 0.0, al = 0.0;
                    if (icemode == 0) ai = ice_single;
                    else if (icemode == 1) ai = absice1[2 * (ki - 1)] + absice1[2 * (ki - 1) + 1] / radice;
                    else if (icemode == 2) { const double *tb = absice2 + 43 * (ki - 1); ai = tb[index_i - 1] + fint_i * (tb[index_i] - tb[index_i - 1]); }
                    else if (icemode == 3) { const double *tb = absice3 + 46 * (ki - 1); ai = tb[index_i - 1] + fint_i * (tb[index_i] - tb[index_i - 1]); }
                    if (liqmode == 0) al = liq_single;
                    else if (liqmode == 1) { const double *tb = absliq1 + 58 * (kl - 1); al = tb[index_l - 1] + fint_l * (tb[index_l] - tb[index_l - 1]); }
                    v = ciwp * ai + clwp * al;
                }
                put(B, v);
            }
        }
    } else if (cf >= cldmin) {
        formed = true;
        // cldprmc on a cloudy sub-column of this layer (the generator gives it the grid-mean values): every band's cell on its own
        const bool water = cwp >= cldmin;
        int ice_err = 0, liq_err = 0, index_i = 1, index_l = 1;
        double radice = 0.0, fint_i = 0.0, fint_l = 0.0;
        bool sized = false;
#pragma unroll 1
        for (int B = 1; B <= NBND; B++) {
            const double tb_in = co_get<R>(a.taucld, co_tau(a, i, k, B - 1));
            double v = tb_in;
            if (water || tb_in >= cldmin) {                                 // cldprmc :181-183 with cldfmc = 1
                if (inflag == 1) err = E_MC_INFLAG1;
                else if (inflag == 2) {
                    if (!sized) {                                           // the table positions (band independent), k_cloudmc's
                        sized = true;
                        if (ciwp != 0.0) {
                            radice = co_get<R>(a.reice, at);
                            if (iceflag == 0) { if (radice < 10.0) ice_err = E_ICE_SMALL; }
                            else if (iceflag == 1) { if (radice < 13.0 || radice > 130.) ice_err = E_ICE_BOUNDS; }
                            else if (iceflag == 2 || iceflag == 3) {
                                const int top = iceflag == 2 ? 43 : 46;
                                if (radice < 5.0 || radice > (iceflag == 2 ? 131.0 : 140.0)) ice_err = iceflag == 2 ? E_ICE_BOUNDS : E_ICE_GEN_BOUNDS;
                                const double factor = (radice - 2.) / 3.;
                                index_i = (int)factor; if (index_i == top) index_i = top - 1;
                                fint_i = factor - (double)index_i;
                                index_i = clampi(index_i, 1, top - 1);
                            }
                        }
                        if (clwp != 0.0 && liqflag == 1) {
                            const double radliq = co_get<R>(a.reliq, at);
                            if (radliq < 2.5 || radliq > 60.) liq_err = E_LIQ_BOUNDS;
                            index_l = (int)(radliq - 1.5);
                            if (index_l == 0) index_l = 1;
                            if (index_l == 58) index_l = 57;
                            fint_l = radliq - 1.5 - (double)index_l;
                            index_l = clampi(index_l, 1, 57);
                        }
                        if (!err) err = ice_err ? ice_err : liq_err;        // (ice is checked first: cldprmc :204-254)
                    }
                    double ai = 0.0, al = 0.0;
                    if (ciwp != 0.0) {
                        if (iceflag == 0) ai = T.absice0[0] + T.absice0[1] / radice;
                        else if (iceflag == 1) { const int icx = icb_map(B, 1); ai = absice1[2 * (icx - 1)] + absice1[2 * (icx - 1) + 1] / radice; }
                        else if (iceflag == 2) { const double *tb = absice2 + 43 * (B - 1); ai = tb[index_i - 1] + fint_i * (tb[index_i] - tb[index_i - 1]); }
                        else if (iceflag == 3) { const double *tb = absice3 + 46 * (B - 1); ai = tb[index_i - 1] + fint_i * (tb[index_i] - tb[index_i - 1]); }
                    }
                    if (clwp != 0.0) {
                        if (liqflag == 0) al = T.absliq0;
                        else if (liqflag == 1) { const double *tb = absliq1 + 58 * (B - 1); al = tb[index_l - 1] + fint_l * (tb[index_l] - tb[index_l - 1]); }
                    }
                    v = ciwp * ai + clwp * al;
                }
            }
            put(B, v);
        }
    }
    if (err) atomicCAS(a.err, 0, err);
    if (!formed) for (int B = 1; B <= NBND; B++) put(B, 0.0);
}

// ------------------------------------------------------------------------------------------------
// The vertical recurrences: k_sweepc (cloud-free calls and the layers above the batch's highest cloud) and k_sweepz (the cloud zone:
// rtrn, rtrnmr, rtrnmc), below.  Per cell they read k_layer's 4-byte code (cell_code) and form, in float64: transmittance and tfn
// factor (series, or the transmittance table staged in LDS; rtrn :372-451), the layer's Planck functions for the band (setcoef
// :173-269, from tlay / tlev and the band's totplnk row staged in LDS), the Planck fractions (taumol: constant per g-point, or
// interpolated between two fracref rows staged in LDS with the layer's (js, fs) from k_layer) and from them the source terms
// (rtrn :447-449).  The flux contributions (sum over g-points x 0.5 x delwave, rtrn :549-562) are added over a group of bands in LDS
// and written once per group and level.  Lanes beyond the last column work on a copy of the last column; only their stores are masked.
// ------------------------------------------------------------------------------------------------
struct SweepArgs {
    unsigned long long bands;  // the group's bands (all with the same number of quads), one nibble (band - 1) each
    int nbands, ncb;           // number of those bands, number of column blocks (= workgroups)
    int group;                 // index of the group's partial slabs (W.gdn1 ..); split: of its first band's
    int split;                 // 1: a batch that does not fill the chip - grid.y = the group's bands, ONE band per workgroup (a quarter of the
                               // waves per CU, four times the CUs: a level's latency is the dependent issue of one wave, not of three), a slab
                               // per band; k_flux adds the bands of a group first, in the list's order - what the group's workgroup does in LDS
                               // otherwise - so the fluxes do not depend on it
    int ncol, col0, nct, idrv;
    int istart, iend;          // only bands in [istart, iend] are swept
    int cfree;                 // 1 (a cloudy batch of three sweep launches, driver.hip: g_clear_groups): the block groups whose hand-off level is 0 -
                               // no cloudy cell in any of their columns - are swept by a k_sweepc<., 0> launch over the sorted block order and by
                               // no other: a workgroup of that launch leaves unless its group's level is 0, one of the other three if it is
    const double *emis;        // semiss (nct,16)
    const double *cldfrac;     // (nct,nlay)
    const double *tlay;        // (nct,nlay)     layer temperatures    (tlay | tavel)
    const double *tlev;        // (nct,nlay+1)   interface temperatures (tlev | tz)
    // spectral outputs (the sweeps' SPEC instantiations only): per band the flux the band adds to the broadband one, x fluxfac,
    // (nct,nlay+1,16) column fastest - element (i, k, b) at i + nct (k + (nlay + 1) b); clear-sky pair both null or both set
    double *uflxs, *dflxs, *uflxcs, *dflxcs;
};

// index of (column gc, level lvl, band B) in a spectral output array
__device__ __forceinline__ size_t spec_at(size_t gc, int lvl, int B, int nlay, int nct)
{
    return gc + (size_t)nct * ((size_t)lvl + (size_t)(nlay + 1) * (size_t)(B - 1));
}

// LDS of a sweep workgroup: transmittance table (float pairs), per band the Planck rows and the fraction rows
constexpr int SWEEP_LUT_BYTES = 8 * (NTBL + 1) + 8;
constexpr int SWEEP_PL_BYTES = 2 * 184 * 8, SWEEP_FR_BYTES = 16 * 16 * 8;
// Loads of the sweeps: wave-uniform base pointer in a buffer descriptor (scalar registers), per-lane 32-bit byte offset that does not
// change from level to level - no 64-bit vector address arithmetic per load.  nt = streaming (non-temporal) access.
// soff (round 5): the ROW of the level as a wave-uniform 32-bit byte offset in the instruction's scalar-offset operand.  Until then every
// load of a level formed its row's 64-bit address (clamp, a signed 64-bit multiply by the row stride, the add, the descriptor's second
// word: ~14 scalar instructions, ~106 per level and thread in k_sweepz), and the scalar stream is NOT hidden behind the vector one at
// three waves per SIMD: 100 scalar instructions more per level cost the sweeps 10 % (measured with a knock-in, n more dependent scalar
// additions per level and thread: profiles/round5_instruction_diet.md).
// Now the descriptor is built from the array's start (the compiler keeps it across the level loop) and a level costs the workspace arrays
// one multiply for the row and a shift per element size; the rows of the caller's arrays, whose column stride is the whole call's column
// count, keep a 64-bit address, formed from an unsigned 32 x 32 -> 64 bit product (row_ptr).  The driver keeps the end of every row inside
// the descriptor's 0x7ffffff0 bytes (driver.hip: eff_batch, SWEEP_RANGE).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sweep_rsrc(const void *base)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, 0x7ffffff0, 0x00020000);
}
// a quad record of cell codes (voff = the lane's column x CODE_BYTES), streaming
__device__ __forceinline__ pk4 bload_pk4_nt(const void *base, unsigned voff, unsigned soff = 0u)
{
    pk4 r;
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(sweep_rsrc(base), (int)voff, (int)soff, 2);
    __builtin_memcpy(&r, &v, 16);
    return r;
}
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double bload_f64(const void *base, unsigned voff, unsigned soff = 0u)
{
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(sweep_rsrc(base), (int)voff, (int)soff, 0);
    double r;
    __builtin_memcpy(&r, &v, 8);
    return r;
}
__device__ __forceinline__ double2 bload_f64x2(const void *base, unsigned voff, unsigned soff = 0u)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(sweep_rsrc(base), (int)voff, (int)soff, 0);
    double2 r;
    __builtin_memcpy(&r, &v, 16);
    return r;
}
__device__ __forceinline__ unsigned bload_u32(const void *base, unsigned voff, unsigned soff = 0u)
{
    return __builtin_amdgcn_raw_buffer_load_b32(sweep_rsrc(base), (int)voff, (int)soff, 0);
}
// row `r` of a caller's (column-fastest) array whose rows lie `stride` doubles apart: a 64-bit address from an unsigned 32 x 32 product
__device__ __forceinline__ const double *row_ptr(const double *base, unsigned r, unsigned stride)
{
    return base + (unsigned long long)r * (unsigned long long)stride;
}

__device__ __forceinline__ void bstore_f64(void *base, unsigned voff, double v)
{
    u32x2 x;
    __builtin_memcpy(&x, &v, 8);
    __builtin_amdgcn_raw_buffer_store_b64(x, sweep_rsrc(base), (int)voff, 0, 0);
}
__device__ __forceinline__ void bstore_f64x2(void *base, unsigned voff, double v0, double v1)
{
    const double t[2] = {v0, v1};
    u32x4 x;
    __builtin_memcpy(&x, t, 16);
    __builtin_amdgcn_raw_buffer_store_b128(x, sweep_rsrc(base), (int)voff, 0, 0);
}

// table index of a cell's code (0 for the series branch: entry 0 is {1 - exp = 0, tfn = 0})
// From here to the end of k_sweepz nothing is contracted behind the source's back: every fused multiply-add of the sweeps is written as
// one (fma).  The two sweep kernels, and the copies of a level's body inside each (one per prefetch slot), must round a level alike -
// which of them sweeps a level follows from the clouds of the 64-column block a column shares - and with contraction left to the
// compiler they did not: tp + f * (tq1 - tq0) of planck_at fused in one inlined copy and not in another moved a flux partial by an ulp
// (tools/soak_host_entry.py, tests/test_hip_parity.py::test_a_column_does_not_depend_on_its_neighbours).
#pragma clang fp contract(off)
__device__ __forceinline__ unsigned code_index(scr_t c) { return (unsigned)max((int)(-c), 0); }
// the optical depth of a series cell, 0 for a table cell: max(c, 0) on the bit pattern (a negative float is a negative integer)
__device__ __forceinline__ float code_od(scr_t c) { return __int_as_float(max(__float_as_int(c), 0)); }
// (1 - transmittance, tfn factor) of a cell from its code and the table entry at code_index: rtrn :439-451.  Branch-free: a table
// cell adds the series terms of od = 0, a series cell adds the table terms of entry 0 - both exact zeros.  Float arithmetic up to the
// two conversions (decode_f32: the part in float): the table values are floats already, and of the two summands one is an exact
// zero; the series terms carry ~1e-7 relative error (od <= 0.06), the same class as the float table entries.  (A float64
// form of the same three operations was carried beside this one as a build switch and never selected; no profile holds numbers for it.)
__device__ __forceinline__ void decode_f32(scr_t c, const float2 &e, float &atr, float &tfn)
{
    const float od = code_od(c);
    atr = e.x + __builtin_fmaf(-0.5f * od, od, od);
    tfn = __builtin_fmaf(0.166667f, od, e.y);
}
__device__ __forceinline__ void decode(scr_t c, const float2 &e, double &atr, double &tfn)
{
    float fa, ft;
    decode_f32(c, e, fa, ft);
    atr = (double)fa;
    tfn = (double)ft;
}
// Records that are all thin.  Above the clouds 96 % of the cells are series cells, and 89 % of the quad records a wave loads with one
// 16-byte access hold series cells in all 64 lanes (profiles/sweepc_thin_records.md).  For those the table side of decode() - the index,
// the LDS address, the gathered read of entry 0 = {0, 0}, the clamp and the two additions of zero - produces nothing.  k_sweepc tests
// per record whether every code of the wave has its sign bit clear and then takes decode_thin.  (decode() for every record, the body before
// this one, was 57.85 against 56.75 ms a step; the downward phase above the clouds does not lose with the thin body and needed no choice
// of its own: profiles/sweepc_thin_records.md.)  One test per thread and level
// over all of its records, with two straight-line bodies, spilled registers in the downward phase of the 12- and 16-g-point bands and
// was not kept.
// decode_f32() of a series cell (sign bit of the code clear: the code is the optical depth, code_index is 0).  Rounds like decode_f32():
// there e.x = +0.0f is added to a float that is never negative (od <= 0.06) and comes out +0 at od = 0 - the sum is that float, bit for
// bit - and fmaf(0.166667f, od, +0.0f) rounds the one product 0.166667f * od; the float denormal mode is the same for all of these.
__device__ __forceinline__ void decode_thin(scr_t od, float &atr, float &tfn)
{
    atr = __builtin_fmaf(-0.5f * od, od, od);
    tfn = 0.166667f * od;
}
// no code of the wave's lanes in these records is a table code: a wave-uniform (scalar) condition, the exec mask stays whole.  A negative
// float - a table code, -0.0f included - is a negative integer.
__device__ __forceinline__ bool wave_all_thin(unsigned orw) { return __builtin_amdgcn_ballot_w64((int)orw < 0) == 0ull; }
// (The table entry evaluated instead of looked up - the closed forms rrtmg_lw_ini tabulates, src/rrtmg_lw_init.f90:125-142, in float32
// with the hardware exp2 / rcp - frees the table's 80 KB of LDS and costs ~12 more instructions per cell, 4 of them transcendental, and
// float32 cancellation in 1 - exp and in tfn.  Measured and not kept: profiles/round2_n1_expf.md.)

// integrated Planck function at temperature t from one band's row of totplnk: setcoef :173-269
__device__ __forceinline__ double planck_at(const double *tp, const double *tq, double t)
{
    const double x = t - 159.;
    const int ind = clampi((int)x, 1, 180);
    const double f = x - (double)ind;
    return fma(f, tq[ind] - tq[ind - 1], tp[ind - 1]);
}

// LDS tables of a sweep workgroup (one band): the transmittance table as float pairs {1 - exp, tfn}, the band's row of totplnk (and band
// 16's, for the istart = 16 variant of setcoef :233-246), its Planck-fraction rows (0-8 fracrefa, 9-13 fracrefb, 14-15 zeros).  Ends
// with a barrier.
__device__ __forceinline__ void sweep_stage_lut(const DevTables &T, unsigned char *smem, int tid, int nth)
{
    const double2 *src = reinterpret_cast<const double2 *>(T.stat + T.sl.lutf);
    double2 *dst = reinterpret_cast<double2 *>(smem);
    // (loads first, then the LDS writes, eight at a time: a plain copy loop waits for every load before it issues the next)
    constexpr int NLUT = SWEEP_LUT_BYTES / 16;
    for (int i0 = tid; i0 < NLUT; i0 += 8 * nth) {
        double2 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = src[min(i0 + k * nth, NLUT - 1)];
#pragma unroll
        for (int k = 0; k < 8; k++) if (i0 + k * nth < NLUT) dst[i0 + k * nth] = v[k];
    }
}
// one band's Planck integrals and Planck-fraction rows
__device__ __forceinline__ void sweep_stage_band(const DevTables &T, double (*s_pl)[184], double (*s_fr)[16], int B, bool alt16, bool lo_bin, bool up_bin,
                                                 int tid, int nth)
{
    const double *tp = alt16 ? T.stat + T.sl.totplk16 : T.stat + T.sl.totplnk + 181 * (B - 1);
    const double *tq = T.stat + T.sl.totplnk + 181 * 15;
    for (int i = tid; i < 181; i += nth) { s_pl[0][i] = tp[i]; s_pl[1][i] = tq[i]; }
    const int ng = T.band[B - 1].ng, fa = T.band[B - 1].fracrefa, fb = T.band[B - 1].fracrefb;
    const int na = lo_bin ? 9 : 1, nb = up_bin ? 5 : 1;
    for (int i = tid; i < 16 * 16; i += nth) {
        const int r = i >> 4, g = i & 15;
        double v = 0.0;
        if (g < ng) {
            if (r < 9) { if (r < na) v = T.ktab[fa + r * ng + g]; }
            else if (r < 14 && fb >= 0 && r - 9 < nb) v = T.ktab[fb + (r - 9) * ng + g];
        }
        s_fr[r][g] = v;
    }
}
// ------------------------------------------------------------------------------------------------
// k_sweepc : the clear-sky recurrences (src/rrtmg_lw_rtrn.f90:437-466 downward, :497-540 upward; identical in rtrnmr / rtrnmc) with
//            ALL g-points of a band in one thread: one thread = (column, band), no reduction across threads.  The work of a level that
//            does not depend on the g-point (two Planck interpolations, fraction-row selection, the loads of temperatures and codes,
//            loop control) is done once for up to 16 g-points instead of once per quad, and the wave has up to 16 independent
//            recurrences in flight.
//   PHASE 0  the whole column of a cloud-free call (icld = 0): downward, surface (rtrn :476-495), upward
//   PHASE 1  layers ltop+1 .. nlay downward, for the cloudy modes: above its block's hand-off level ltop (W.hgrp, k_blocksort) every column
//            of a wave is clear and the clear-sky stream equals the total one; the radiances at level ltop go to k_sweepz through W.hand
//   PHASE 2  layers ltop+1 .. nlay upward, total and clear-sky streams, starting from the radiances k_sweepz left in W.hand
// ------------------------------------------------------------------------------------------------
// waves per SIMD each instantiation is compiled for = what its registers allow without spilling (a spilled register is reloaded with a
// scratch load, which counts as a vector-memory operation: its wait drains every prefetch in flight), at most 4 (one workgroup of
// <= 1024 threads per CU: the transmittance table takes half of the LDS).  Register needs, unconstrained, by quads per thread 4 / 3 / 2 / 1:
//   phase 1                       154 148 102  84          (as compiled since the fused multiply-adds are written out: 136 114  91  75)
//   phase 0                       247 171 147 106          (two waves per band at 4 quads: 112; 140 111  85)
//   phase 2                       256+ 222 172 102         (145 with two waves per band; 188 143  95)
//   phase 0 with d/dT             250 199 148 105          (146; 189 144  95)
//   phase 2 with d/dT             256+ 256+ 241 132        (212; 256 + 44 accumulation registers; 210 126)
#ifndef RRLW_SWEEPC_P0
#define RRLW_SWEEPC_P0 6, 4, 3, 2      // (6, 3, 2, 2 until the sweeps' fused multiply-adds were written out: 111 / 140 registers at 2 / 3 quads since; 1e4 clear columns 0.78 -> 0.69 ms)
#endif
#ifndef RRLW_SWEEPC_P2D
#define RRLW_SWEEPC_P2D 3, 2, 1, 1
#endif
#ifndef RRLW_SWEEPC_WAVES_CAP
#define RRLW_SWEEPC_WAVES_CAP 4
#endif
__host__ __device__ constexpr int sweepc_waves(int NQ, int PHASE, bool IDRV)
{
    const int row = PHASE == 1 ? 0 : (PHASE == 0 && !IDRV) ? 1 : (PHASE == 2 && IDRV) ? 3 : 2;
    const int tab[4][4] = {{7, 5, 4, 3}, {RRLW_SWEEPC_P0}, {5, 3, 2, 1}, {RRLW_SWEEPC_P2D}};      // [row][NQ - 1]
    const int w = tab[row][NQ - 1];
    return w < RRLW_SWEEPC_WAVES_CAP ? w : RRLW_SWEEPC_WAVES_CAP;
}
// A workgroup = the bands of one GROUP (threadIdx.y; all with NQ quads) x column sub-blocks of 64 (threadIdx.z), one workgroup per CU
// (the transmittance table takes half of the LDS).  The per-level partials of the group's bands are added in LDS, in the order of the
// group's band list, every RRLW_SWEEPC_CODES levels: one 8- or 16-byte partial per group, level and column goes to HBM instead of one
// per band (16 bands -> 4 groups: the partial slabs were a quarter of this kernel's traffic and all of k_flux's).
constexpr int NGROUP_MAX = 8;
constexpr int SWEEPC_BAND_BYTES = SWEEP_PL_BYTES + SWEEP_FR_BYTES;
// values per band, level and column in the reduction buffer: total [, clear] [, their d/dT]
__host__ __device__ constexpr int sweepc_nval(int PHASE, bool IDRV) { return (PHASE == 2 ? 2 : 1) * ((IDRV && PHASE != 1) ? 2 : 1); }
#ifndef RRLW_SWEEPC_CODES
#define RRLW_SWEEPC_CODES 2       // code slots: levels of cell codes in flight (the codes are the one HBM stream of the sweep; 4 registers per quad and slot)
#endif
constexpr int SWEEPC_LDS_MAX = 160 * 1024;
__host__ __device__ constexpr int sweepc_lds_bytes(int PHASE, bool IDRV, int nb, int nsb, int NT = 1)
{
    return SWEEP_LUT_BYTES + nb * SWEEPC_BAND_BYTES + 2 * sweepc_nval(PHASE, IDRV) * nb * NT * RRLW_SWEEPC_CODES * nsb * 64 * 8;
}
// threads per band: two where a band's 16 g-points with two streams would otherwise leave one wave per SIMD
__host__ __device__ constexpr int sweepc_nt(int NQ, int PHASE)
{
    // 12 g-points x {total, clear} x {radiance, d/dT} in one thread need 256 registers + 70 accumulation registers as spill space: one wave
    // per SIMD.  Three threads of one quad (three waves per SIMD, nothing spilled) repeat the level's Planck terms, fraction rows and
    // temperature loads three times: 8.26 ms against 5.59 per 5e5 137-layer columns - the one-wave form stays.  (The downward clear-sky
    // sweep of the 16-g-point bands on two threads as well was measured too and stays on one.)
    return (NQ == 4 && (PHASE == 2 || PHASE == 0)) ? 2 : 1;
}
// bands per group: what fits the wave slots of the most register-hungry instantiation (phase 2 with d/dT)
__host__ __device__ constexpr int sweepc_group_cap(int NQ)
{
    int cap = 5;
    for (int ph = 0; ph < 3; ph++)
        for (int i = 0; i < 2; i++) {
            if (ph == 1 && i == 1) continue;
            const bool idrv = i == 1;
            const int nt = sweepc_nt(NQ, ph), w = 4 * sweepc_waves(NQ / nt, ph, idrv) / nt;      // wave slots
            if (w < cap) cap = w;
            while (cap > 1 && sweepc_lds_bytes(ph, idrv, cap, 1, nt) > SWEEPC_LDS_MAX) cap--;           // reduction buffer
        }
    return cap;
}
// column sub-blocks per workgroup for a group of nb bands
__host__ __device__ constexpr int sweepc_nsb(int NQ, int PHASE, bool IDRV, int nb)
{
    const int nt = sweepc_nt(NQ, PHASE);
    int nsb = nsb_fit(4 * sweepc_waves(NQ / nt, PHASE, IDRV) / (nb * nt));         // (a divisor of SORT_GROUP: workgroups never straddle hand-off groups)
    while (nsb > 1 && sweepc_lds_bytes(PHASE, IDRV, nb, nsb, nt) > SWEEPC_LDS_MAX) nsb = nsb_fit(nsb - 1);
    return nsb;
}

// One slot of the rolling prefetch.  Every load is issued on every path (rows clamped to 1 .. nlay instead of skipped): the compiler can
// then count the loads in flight behind the one it needs and wait with vmcnt(N) instead of vmcnt(0) - vector-memory operations complete
// in order, so a wait for everything would stall the wave on the codes it has just requested for the next level.
template <int G> struct SweepcLev { double tl, tz; unsigned w; };

// 1 - x as a value of its own.  With contraction allowed across statements the compiler folds (1 - x) * y into fma(-x, y, y) where the
// difference has a single use and keeps the product where it has several: the same source line then rounds differently in two copies of
// the level body (the two prefetch slots, the two kernels) and a level's d(flux)/dT depended, in its last bit, on the hand-off level of
// its block - found by tools/soak_host_entry.py.  The empty asm hides the subtraction from that fold.
__device__ __forceinline__ double one_minus(double x)
{
    double t = 1.0 - x;
    asm("" : "+v"(t));
    return t;
}
// ... and a product as a value of its own: d(radiance)/dT of a level is the product radiance' x (1 - a), which is both the state carried
// upward and a term of the level's sum over the g-points - fused into that sum (fma(radiance', 1 - a, next term)) in one copy of the body
// and not in another, the sum rounded differently.  (The radiances themselves are results of an fma; nothing is left to fuse.)
__device__ __forceinline__ double times(double x, double y)
{
    double t = x * y;
    asm("" : "+v"(t));
    return t;
}

// NT threads (waves) per band, each with G = NQ / NT of its quads: the band's partial is the sum of their raw quad sums, formed - with the
// band's weight - by the wave that adds the group (so a band split over two waves still rounds like one swept by a single thread).  Used
// where all 16 g-points of a band with two streams would leave one wave per SIMD (sweepc_nt).
// SPEC: each band's flux of a level also goes, x fluxfac, to the caller's spectral arrays (SweepArgs::uflxs ..) at the lane's column.
template <int NQ, int PHASE, bool IDRV, int NT = 1, bool SPEC = false>
__global__ __launch_bounds__(256 * sweepc_waves(NQ / NT, PHASE, IDRV), sweepc_waves(NQ / NT, PHASE, IDRV)) void k_sweepc(DevTables T, Workspace W, SweepArgs a)
{
    static_assert(NQ % NT == 0 && (NT == 1 || NT == 2), "threads per band");
    constexpr int G = NQ / NT, NG = 4 * G, NC = RRLW_SWEEPC_CODES;
    constexpr bool DOWN = PHASE != 2, UP = PHASE != 1, TWO = PHASE == 2;       // TWO: total and clear-sky streams differ
    constexpr int NVAL = sweepc_nval(PHASE, IDRV);
    extern __shared__ __align__(16) unsigned char smem[];
    // The hand-off level of the workgroup's block group (it never straddles two groups): ONE scalar load, taken before anything is staged.
    // Cloud-free groups of a cloudy batch (SweepArgs::cfree) belong to phase 0 and to no other phase.  (A cloud-free call has no groups.)
    const int hgrp = (PHASE == 0 && !a.cfree) ? 0 : __builtin_amdgcn_readfirstlane(W.hgrp[(blockIdx.x * blockDim.z) / SORT_GROUP]);
    if (a.cfree && (PHASE == 0) != (hgrp == 0)) return;
    // (a wave = 64 consecutive threadIdx.x of one (y, z): band and sub-block are wave-uniform - made scalar, so that everything derived
    // from the band, buffer descriptors included, lives in scalar registers)
    const int tx = threadIdx.x, ty = __builtin_amdgcn_readfirstlane(threadIdx.y), sub = __builtin_amdgcn_readfirstlane(threadIdx.z);
    const int bi = ty / NT, part = ty % NT;                                     // band of the group, part of the band
    const int ny = blockDim.y, nb = ny / NT, nsb = blockDim.z, ncw = 64 * nsb;  // waves per column sub-block, bands of the group, sub-blocks, columns of the workgroup
    const float2 *s_lut = reinterpret_cast<const float2 *>(smem);
    double (*s_pl)[184] = reinterpret_cast<double (*)[184]>(smem + SWEEP_LUT_BYTES + bi * SWEEPC_BAND_BYTES);
    double (*s_fr)[16] = reinterpret_cast<double (*)[16]>(smem + SWEEP_LUT_BYTES + bi * SWEEPC_BAND_BYTES + SWEEP_PL_BYTES);
    double *red = reinterpret_cast<double *>(smem + SWEEP_LUT_BYTES + nb * SWEEPC_BAND_BYTES);      // [2][NVAL][nb][NC][ncw]
    // the wave's 64-column block: position (workgroup, sub-block) of the order k_blocksort left (deepest clouds first); a cloud-free call
    // (PHASE 0 without cfree) has no order and takes the blocks as they come
    const int slot = blockIdx.x * nsb + sub;
    const int cblock = (PHASE == 0 && !a.cfree) ? slot : __builtin_amdgcn_readfirstlane(W.order[slot]);
    const int col = cblock * 64 + tx;
    const int bsel = a.split ? (int)blockIdx.y : 0;                             // split: this workgroup's band of the group
    const unsigned long long bands = a.bands >> (4 * bsel);
    const int B = (int)((bands >> (4 * bi)) & 15ull) + 1;
    const bool incol = col < a.ncol;
    const int colc = incol ? col : a.ncol - 1;
    const int quad = __builtin_amdgcn_readfirstlane(band_qstart(B) + part * G);
    const int g0 = NG * part;                                                   // first of this thread's g-points within the band
    const int pc = pcol(W, colc);                                               // the column at this position (caller arrays)
    const size_t gc = (size_t)a.col0 + pc;
    const int nlay = W.nlay, nct = a.nct;
    const size_t ncb = W.ncolb;
    const bool alt16 = (B == 16 && a.istart == 16);
    const bool lo_bin = (LO_BINARY >> (B - 1)) & 1u, up_bin = (UP_BINARY >> (B - 1)) & 1u;
    const bool any_bin = lo_bin || up_bin;
    const int base_up = ((UP_ZERO >> (B - 1)) & 1u) ? 14 : (((UP_FROM_A >> (B - 1)) & 1u) ? 0 : 9);
    sweep_stage_lut(T, smem, (sub * ny + ty) * 64 + tx, 64 * ny * nsb);
    sweep_stage_band(T, s_pl, s_fr, B, alt16, lo_bin, up_bin, (sub * NT + part) * 64 + tx, NT * ncw);
    __syncthreads();
    const int lo = PHASE == 0 ? 1 : hgrp + 1;       // layers lo .. nlay (uniform over the workgroup)
    const size_t qstride = (size_t)nlay * ncb;
    const unsigned *__restrict__ sC = W.scr[S_CODE] + (size_t)quad * qstride * CODE_WORDS;
    const unsigned *__restrict__ sFw = W.fw + (size_t)fw_slot(B) * nlay * ncb;
    // (temperatures: the caller's rows - or, for a window whose columns are taken in another order, their copies in position order: the
    // lane's offset is its position either way, eight consecutive bytes per lane)
    const bool moved = pmoved(W, colc);
    const double *__restrict__ tlay = moved ? W.tlayc : a.tlay + a.col0;
    const double *__restrict__ tlev = moved ? W.tlevc : a.tlev + a.col0;
    const size_t tstride = moved ? ncb : (size_t)nct;
    const unsigned offc = (unsigned)colc * (unsigned)CODE_BYTES, off8p = (unsigned)colc * 8u, off4 = (unsigned)colc * 4u;
    const size_t pcb = (size_t)W.pcb;
    const size_t gslab = (size_t)(a.group + bsel) * (nlay + 1) * pcb;        // (uniform: the group's slabs; a lane's column is the 32-bit offset of a buffer store)
    double *__restrict__ gdn1 = W.gdn1 + gslab;
    double *__restrict__ gup1 = W.gup1 + gslab;
    Part2 *__restrict__ gup = W.gup + gslab;
    Part2 *__restrict__ gdp = W.gdp + gslab;
    const unsigned so8 = (unsigned)col * 8u, so16 = (unsigned)col * 16u;
    const int laytrop = W.laytrop[colc];
    const double *tp0 = s_pl[0], *tp1 = s_pl[1];
    double2 *hand = reinterpret_cast<double2 *>(W.hand) + ((size_t)quad * ncb + colc) * 2;      // [stream][quad][column][2]
    const size_t hstream = (size_t)NQUAD * ncb * 2;

    // loads of layer `lev` (any integer: rows outside 1 .. nlay are clamped, their values never used); zoff selects the interface whose
    // temperature the sweep direction needs: 0 = level lev - 1 (below the layer, downward sweep), 1 = level lev (above, upward sweep)
    // (rows as scalar offsets - bload_*'s soff - in the two-stream phases, which are bound by instruction issue: -1.5 %.  The downward
    // phase above the clouds streams at the memory pipeline's rate and lives by WHERE its code loads sit in the level body; with the
    // lighter address arithmetic the scheduler gathers them at the end of the body, the prefetch distance shrinks and the phase takes 3 %
    // longer (profiles/round5_instruction_diet.md): it keeps the row addresses it had.)
    constexpr bool SOFF = PHASE != 1;
    const unsigned ncb32 = (unsigned)ncb, tstr32 = (unsigned)tstride;
    auto fill_t = [&](auto bin_tag, int lev, int zoff, SweepcLev<G> &q) {
        const int l = min(max(lev, 1), nlay);
        if constexpr (SOFF) {
            const unsigned r = (unsigned)(l - 1);
            q.tl = bload_f64(row_ptr(tlay, r, tstr32), off8p);
            q.tz = bload_f64(row_ptr(tlev, r + (unsigned)zoff, tstr32), off8p);
            if constexpr (decltype(bin_tag)::value) q.w = bload_u32(sFw, off4, r * ncb32 * 4u);
        } else {
            q.tl = bload_f64(tlay + tstride * (l - 1), off8p);
            q.tz = bload_f64(tlev + tstride * (l - 1 + zoff), off8p);
            if constexpr (decltype(bin_tag)::value) q.w = bload_u32(sFw + (size_t)(l - 1) * ncb, off4);
        }
    };
    auto ld_c = [&](int lev, int k) -> pk4 {
        const int l = min(max(lev, 1), nlay);
        if constexpr (SOFF) return bload_pk4_nt(sC + (size_t)k * qstride * CODE_WORDS, offc, (unsigned)(l - 1) * ncb32 * (unsigned)CODE_BYTES);
        else return bload_pk4_nt(sC + ((size_t)k * qstride + (size_t)(l - 1) * ncb) * CODE_WORDS, offc);
    };
    // fraction rows of layer `lev`: first row and interpolation weight (taumol :556-561, :692-693)
    auto frac_row = [&](int lev, unsigned fwv, double &fpl) -> const double * {
        const bool lower = lev <= laytrop;
        if (any_bin) {          // uniform
            const unsigned w = (lower ? lo_bin : up_bin) ? fwv : 0x10000000u;
            const int r0 = clampi((lower ? 0 : base_up) + (int)(w >> 28) - 1, 0, 14);
            fpl = (double)(w & 0x0fffffffu) * (1.0 / 268435456.0);
            return &s_fr[r0][g0];
        }
        fpl = 0.0;
        return &s_fr[lower ? 0 : base_up][g0];
    };

    // A wave's raw sum over its g-points of a level goes to the reduction buffer [buffer][value][wave][slot][column]; after the NC levels of a
    // round the workgroup meets at ONE barrier, wave `ty` forms the bands' partials of slot ty (ty + ny, ..) - (sum of the band's waves x 0.5)
    // x delwave, rtrn :549-562 - adds them in band-list order and stores the group's partial.  Two buffers: the next round writes the other
    // one, and a buffer is written again only after the barrier in between, which no wave passes before every wave has finished reading it.
    const unsigned rlane = (unsigned)(sub * 64 + tx);
    const unsigned vstride = (unsigned)(ny * NC * ncw), rband = (unsigned)(ty * NC * ncw);      // (uniform)
    unsigned bufoff = 0u;                                                                       // 0 / NVAL * vstride
    auto red_put = [&](int c, int val, double v) { red[bufoff + val * vstride + rband + (unsigned)(c * ncw) + rlane] = v; };
    auto round_end = [&](auto dn_tag, int lev0, int nvalid) {
#pragma clang fp contract(off)      // (a band's weight, the flux factor and the sum over the bands round as written: in k_sweepz too - a level's partial must not depend on the kernel that swept it)
        constexpr bool DN = decltype(dn_tag)::value;
        constexpr int NV = DN ? 1 : NVAL;
        __syncthreads();
        for (int c = ty; c < nvalid; c += ny) {       // (wave-uniform)
            const int lvl = DN ? lev0 - c - 1 : lev0 + c;
            double sv[NV];
#pragma unroll
            for (int val = 0; val < NV; val++) {
                const double *r = red + (bufoff + val * vstride + (unsigned)(c * ncw) + rlane);
                const bool deriv = IDRV && !DN && val >= (TWO ? 2 : 1);
                double sum = 0.0;
                for (int q = 0; q < nb; q++) {
                    double pq = r[(unsigned)(q * NT * NC * ncw)];            // (the band's parts in the order one thread adds its quads: pairs first)
                    if constexpr (NT == 2) pq = pq + r[(unsigned)((q * NT + 1) * NC * ncw)];
                    const int bq = (int)((bands >> (4 * q)) & 15ull);
                    double v = (pq * 0.5) * T.delwave[bq];
                    if (deriv) v = v * T.fluxfac;
                    sum = q == 0 ? v : sum + v;
                    if constexpr (SPEC) {
                        // one stream downward and in a cloud-free call: the clear-sky arrays take the same value
                        if (incol && !deriv) {
                            const size_t o = spec_at(gc, lvl, bq + 1, nlay, nct);
                            const double f = v * T.fluxfac;
                            if (DN) { a.dflxs[o] = f; if (a.dflxcs) a.dflxcs[o] = f; }
                            else if (val == 0) { a.uflxs[o] = f; if (!TWO && a.uflxcs) a.uflxcs[o] = f; }
                            else if (a.uflxcs) a.uflxcs[o] = f;
                        }
                    }
                }
                sv[val] = sum;
            }
            if (incol) {
                if constexpr (DN) bstore_f64(gdn1 + (size_t)lvl * pcb, so8, sv[0]);
                else {
                    if constexpr (TWO) bstore_f64x2(gup + (size_t)lvl * pcb, so16, sv[0], sv[1]);
                    else bstore_f64(gup1 + (size_t)lvl * pcb, so8, sv[0]);
                    if constexpr (IDRV) bstore_f64x2(gdp + (size_t)lvl * pcb, so16, TWO ? sv[2] : sv[1], TWO ? sv[3] : sv[1]);
                }
            }
        }
        bufoff = bufoff ? 0u : NVAL * vstride;
    };

    double rad[NG], radc[TWO ? NG : 1], drad[IDRV ? NG : 1], dradc[(IDRV && TWO) ? NG : 1];
#pragma unroll
    for (int j = 0; j < NG; j++) rad[j] = 0.0;

    // One level: layer `lev`, its temperatures in `cur`, its codes in cc[.][lev % NC]; dir = -1 downward (Planck difference towards the
    // interface below, partial of level lev - 1), +1 upward.  BIN: the band's Planck fractions are interpolated between two rows.
    // The slot pieces are re-issued for level lev + NC * dir (codes) / lev + dir (temperatures) as soon as they have been consumed.
    SweepcLev<G> cur;
    cur.w = 0u;
    pk4 cc[G][NC];
    auto level = [&](auto bin_tag, auto dn_tag, int lev, int slot) {
        constexpr bool BIN = decltype(bin_tag)::value, DN = decltype(dn_tag)::value;
        constexpr int dir = DN ? -1 : 1;
        double fpl;
        const double *row = frac_row(lev, cur.w, fpl);
        const double blay = planck_at(tp0, tp0, cur.tl);
        const double dpl = planck_at(tp0, (DN && alt16 && lev == 1) ? tp1 : tp0, cur.tz) - blay;
        fill_t(bin_tag, lev + dir, DN ? 0 : 1, cur);
        // (sums as a tree - pairs inside a quad, then the quads: a running sum over 16 g-points is a chain of 16 dependent additions, and a
        // wave issues in order, so each of them would hold the wave for the latency of the one before)
        double qs[G], qsc[G], qd[G], qdc[G];
        // A record whose codes are series codes in all 64 lanes takes decode_thin - only the transmittance terms sit in the (scalar)
        // branch, the level's loads and the recurrences are common to both sides.
#pragma unroll
        for (int k = 0; k < G; k++) {
            pk4 pk;
#pragma unroll
            for (int c = 0; c < NC; c++) if (c == slot) pk = cc[k][c];
            const scr4 ck = unpack4(pk);
            unsigned orw = pk.w[0];
#pragma unroll
            for (int i = 1; i < CODE_WORDS; i++) orw |= pk.w[i];
            const bool thin = wave_all_thin(orw);
            // (floats across the join, widened behind it: four registers per quad more than the codes they replace)
            float fa[4], ft[4];
            if (thin) {
#pragma unroll
                for (int jj = 0; jj < 4; jj++) decode_thin(ck.v[jj], fa[jj], ft[jj]);
            } else {
                float2 e[4];
#pragma unroll
                for (int jj = 0; jj < 4; jj++) e[jj] = s_lut[code_index(ck.v[jj])];
#pragma unroll
                for (int jj = 0; jj < 4; jj++) decode_f32(ck.v[jj], e[jj], fa[jj], ft[jj]);
            }
            // (behind the branch, where the record's codes have been consumed: issued in front of it, while they are live, the load
            // cannot go to their registers, the slots rotate through copies at the end of a round and those wait for every load)
            const pk4 nx = ld_c(lev + NC * dir, k);
#pragma unroll
            for (int c = 0; c < NC; c++) if (c == slot) cc[k][c] = nx;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int j = 4 * k + jj;
                const double atr = (double)fa[jj], tfn = (double)ft[jj];
                double fr = row[j];
                if constexpr (BIN) fr = fma(fpl, row[16 + j] - fr, fr);
                const double bb = fr * fma(tfn, dpl, blay);
                rad[j] = fma(bb - rad[j], atr, rad[j]);
                if constexpr (TWO && !DN) radc[j] = fma(bb - radc[j], atr, radc[j]);
                if constexpr (IDRV && !DN) {
                    const double tr = one_minus(atr);
                    drad[j] = times(drad[j], tr);
                    if constexpr (TWO) dradc[j] = times(dradc[j], tr);
                }
            }
            qs[k] = (rad[4 * k] + rad[4 * k + 1]) + (rad[4 * k + 2] + rad[4 * k + 3]);
            if constexpr (TWO && !DN) qsc[k] = (radc[4 * k] + radc[4 * k + 1]) + (radc[4 * k + 2] + radc[4 * k + 3]);
            if constexpr (IDRV && !DN) {
                qd[k] = (drad[4 * k] + drad[4 * k + 1]) + (drad[4 * k + 2] + drad[4 * k + 3]);
                if constexpr (TWO) qdc[k] = (dradc[4 * k] + dradc[4 * k + 1]) + (dradc[4 * k + 2] + dradc[4 * k + 3]);
            }
            // (the quad's recurrences stay in front of the next record's branch: sunk behind it - their results are not used before
            // the end of the level - the transmittance terms of every quad of the level are live across the branches, 16 registers
            // per quad.  A scheduling barrier per quad instead - fewer registers, less overlap - was measured slower.)
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                asm volatile("" : "+v"(rad[4 * k + jj]));
                if constexpr (TWO && !DN) asm volatile("" : "+v"(radc[4 * k + jj]));
                if constexpr (IDRV && !DN) asm volatile("" : "+v"(drad[4 * k + jj]));
                if constexpr (IDRV && TWO && !DN) asm volatile("" : "+v"(dradc[4 * k + jj]));
            }
        }
        auto tree = [&](const double (&q)[G]) -> double {
            if constexpr (G == 1) return q[0];
            else if constexpr (G == 2) return q[0] + q[1];
            else if constexpr (G == 3) return (q[0] + q[1]) + q[2];
            else return (q[0] + q[1]) + (q[2] + q[3]);
        };
        red_put(slot, 0, tree(qs));
        if constexpr (TWO && !DN) red_put(slot, 1, tree(qsc));
        if constexpr (IDRV && !DN) {
            red_put(slot, TWO ? 2 : 1, tree(qd));
            if constexpr (TWO) red_put(slot, 3, tree(qdc));
        }
    };
    auto sweep = [&](auto bin_tag, auto dn_tag) {
        constexpr bool DN = decltype(dn_tag)::value;
        constexpr int dir = DN ? -1 : 1;
        const int first = DN ? nlay : lo, count = nlay - lo + 1;
        // (issued in the order the steady state has them in flight at the top of a level - codes of the slots that are older than the
        // level's temperatures, the temperatures, the youngest slot - so that the waits of the loop header can be counted ones)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c == NC - 1) fill_t(bin_tag, first, DN ? 0 : 1, cur);
#pragma unroll
            for (int k = 0; k < G; k++) cc[k][c] = ld_c(first + c * dir, k);
        }
        int n = 0;
        for (; n + NC <= count; n += NC) {          // whole rounds of NC levels: a straight-line body (a skipped level inside the loop makes
#pragma unroll                                      // the compiler rotate the slot registers through copies, which wait for every load)
            for (int c = 0; c < NC; c++) level(bin_tag, dn_tag, first + (n + c) * dir, c);
            round_end(dn_tag, first + n * dir, NC);
        }
        const int rem = count - n;                  // (uniform over the workgroup)
#pragma unroll
        for (int c = 0; c < NC - 1; c++) {
            if (c < rem) level(bin_tag, dn_tag, first + (n + c) * dir, c);
        }
        if (rem > 0) round_end(dn_tag, first + n * dir, rem);
    };
    using std::true_type;
    using std::false_type;

    if constexpr (DOWN) {
        // ------------------------------------------------------------------ downward: layers nlay .. lo
        if (incol && ty == 0) bstore_f64(gdn1 + (size_t)nlay * pcb, so8, 0.0);
        if constexpr (SPEC) {
            if (incol && part == 0) {
                const size_t o = spec_at(gc, nlay, B, nlay, nct);
                a.dflxs[o] = 0.0;
                if (a.dflxcs) a.dflxcs[o] = 0.0;
            }
        }
        if (any_bin) sweep(true_type{}, true_type{}); else sweep(false_type{}, true_type{});
    }
    if constexpr (PHASE == 1) {                     // downward radiances at level ltop for k_sweepz
        if (incol) {
#pragma unroll
            for (int k = 0; k < G; k++) {
                hand[(size_t)k * ncb * 2] = make_double2(rad[4 * k], rad[4 * k + 1]);
                hand[(size_t)k * ncb * 2 + 1] = make_double2(rad[4 * k + 2], rad[4 * k + 3]);
            }
        }
        return;
    }

    if constexpr (PHASE == 0) {
        // ------------------------------------------------------------------ surface: rtrn :476-495
        const double reflect = 1. - a.emis[gc + (size_t)nct * (B - 1)];
        const double pb = W.percol[(size_t)(PC_PLANKBND + B - 1) * ncb + colc];
        const double dpb = IDRV ? W.percol[(size_t)(PC_DPLANKBND + B - 1) * ncb + colc] : 0.0;
        double fpl;
        const double *row = frac_row(1, any_bin ? bload_u32(sFw, off4) : 0u, fpl);        // the surface emits with the lowest layer's Planck fractions
        double usum = 0.0, dusum = 0.0;
#pragma unroll
        for (int j = 0; j < NG; j++) {
            const double fr = any_bin ? fma(fpl, row[16 + j] - row[j], row[j]) : row[j];
            rad[j] = fma(reflect, rad[j], fr * pb);
            usum = usum + rad[j];
            if constexpr (IDRV) { drad[j] = times(fr, dpb); dusum = dusum + drad[j]; }
        }
        if (a.cfree) {
            // In a cloudy batch the surface partial of every other group comes from k_sweepz: one thread per quad adds its four radiances
            // in sequence, round_end the band's quads pairs first.  The same order here - a level's partial must not depend on the path,
            // and batch size decides which blocks share a group.  (A cloud-free call keeps the running sum it has always had.)
            double qs[G], qd[G];
#pragma unroll
            for (int k = 0; k < G; k++) {
                qs[k] = 0.0; qd[k] = 0.0;
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    qs[k] = qs[k] + rad[4 * k + jj];
                    if constexpr (IDRV) qd[k] = qd[k] + drad[4 * k + jj];
                }
            }
            if constexpr (G == 1) { usum = qs[0]; dusum = qd[0]; }
            else if constexpr (G == 2) { usum = qs[0] + qs[1]; dusum = qd[0] + qd[1]; }
            else if constexpr (G == 3) { usum = (qs[0] + qs[1]) + qs[2]; dusum = (qd[0] + qd[1]) + qd[2]; }
            else { usum = (qs[0] + qs[1]) + (qs[2] + qs[3]); dusum = (qd[0] + qd[1]) + (qd[2] + qd[3]); }
        }
        red_put(0, 0, usum);
        if constexpr (IDRV) red_put(0, 1, dusum);
        round_end(false_type{}, 0, 1);              // level 0
    } else {                                        // upward radiances at level ltop from k_sweepz
#pragma unroll
        for (int k = 0; k < G; k++) {
            const double2 *h = hand + (size_t)k * ncb * 2;
            const double2 a0 = h[hstream], a1 = h[hstream + 1], c0 = h[2 * hstream], c1 = h[2 * hstream + 1];
            rad[4 * k] = a0.x; rad[4 * k + 1] = a0.y; rad[4 * k + 2] = a1.x; rad[4 * k + 3] = a1.y;
            if constexpr (TWO) { radc[4 * k] = c0.x; radc[4 * k + 1] = c0.y; radc[4 * k + 2] = c1.x; radc[4 * k + 3] = c1.y; }
            if constexpr (IDRV) {
                const double2 d0 = h[3 * hstream], d1 = h[3 * hstream + 1], e0 = h[4 * hstream], e1 = h[4 * hstream + 1];
                drad[4 * k] = d0.x; drad[4 * k + 1] = d0.y; drad[4 * k + 2] = d1.x; drad[4 * k + 3] = d1.y;
                if constexpr (TWO) { dradc[4 * k] = e0.x; dradc[4 * k + 1] = e0.y; dradc[4 * k + 2] = e1.x; dradc[4 * k + 3] = e1.y; }
            }
        }
    }
    if constexpr (UP) {
        // ------------------------------------------------------------------ upward: layers lo .. nlay
        if (any_bin) sweep(true_type{}, false_type{}); else sweep(false_type{}, false_type{});
    }
}

// ------------------------------------------------------------------------------------------------
// k_sweepz : the cloud zone (layers 1 .. ltop) of the maximum-random-overlap sweep, rtrnmr (src/rrtmg_lw_rtrnmr.f90:509-704), without
//            d(flux)/dT, in k_sweepc's form: one thread = (column, G quads of a band), a workgroup = the bands of one group, every load
//            issued on every path (the cloudy level's extra inputs - total-optical-depth codes, cloud fraction, overlap factors - are
//            read for every level of the zone) so that the waits are counted ones, partials added over the group in LDS every two
//            levels, ONE barrier per round.  A wave none of whose 64 columns is cloudy at a level runs the clear-sky body; otherwise
//            both updates are formed and selected per lane (what divergence does anyway).  Its predecessor k_sweep (one workgroup per band, removed) did the same work at
//            1.9x the time per clear level (per-quad duplication of the level's Planck terms, conditional loads with full waits, two
//            barriers per four levels).
// ------------------------------------------------------------------------------------------------
// One quad per thread, so a band of NQ quads takes NQ threads (waves).  (Two quads per thread for the bands of 4 and 2 quads: 253
// registers, two waves per SIMD - measured slower.)
__host__ __device__ constexpr int sweepz_nt(int NQ) { return NQ; }
#ifndef RRLW_SWEEPZ_WAVES_G1
#define RRLW_SWEEPZ_WAVES_G1 3
#endif
#ifndef RRLW_SWEEPZ_WAVES_IDRV
#define RRLW_SWEEPZ_WAVES_IDRV 2          // with d(flux)/dT: 16 more state registers per thread
#endif
__host__ __device__ constexpr int sweepz_waves(int /* NQ */, bool IDRV = false)
{
    return IDRV ? RRLW_SWEEPZ_WAVES_IDRV : RRLW_SWEEPZ_WAVES_G1;
}
__host__ __device__ constexpr int sweepz_lds_bytes(int nb, int nsb, int NT, bool IDRV = false)
{
    return SWEEP_LUT_BYTES + nb * SWEEPC_BAND_BYTES + 2 * (IDRV ? 4 : 2) * nb * NT * RRLW_SWEEPC_CODES * nsb * 64 * 8;
}
__host__ __device__ constexpr int sweepz_nsb(int NQ, int nb, bool IDRV = false)
{
    const int nt = sweepz_nt(NQ);
    int nsb = nsb_fit(4 * sweepz_waves(NQ, IDRV) / (nb * nt));
    while (nsb > 1 && sweepz_lds_bytes(nb, nsb, nt, IDRV) > SWEEPC_LDS_MAX) nsb = nsb_fit(nsb - 1);
    return nsb;
}

// bands per group: wave slots and LDS of one workgroup
__host__ __device__ constexpr int sweepz_group_cap(int NQ, bool IDRV)
{
    const int nt = sweepz_nt(NQ);
    int cap = 4 * sweepz_waves(NQ, IDRV) / nt;
    if (cap < 1) cap = 1;
    while (cap > 1 && sweepz_lds_bytes(cap, 1, nt, IDRV) > SWEEPC_LDS_MAX) cap--;
    return cap;
}

struct SweepzLev { double tl, tz, cf; unsigned w, flag; };

// MODE: 1 rtrn (random overlap), 2 rtrnmr, 3 rtrnmc with per-g-point arrays, 4 rtrnmc with the generator's sub-column mask
// IDRV: d(upward flux)/dT carried along (idrv = 1), src/rrtmg_lw_rtrnmr.f90:655-703 and its siblings
// SPEC: as in k_sweepc, every band's flux of a level also goes to the caller's spectral arrays
template <int NQ, int MODE, bool IDRV = false, bool SPEC = false>
__global__ __launch_bounds__(256 * sweepz_waves(NQ, IDRV), sweepz_waves(NQ, IDRV)) void k_sweepz(DevTables T, Workspace W, SweepArgs a)
{
    static_assert(MODE >= 1 && MODE <= 4, "modes of the cloud-zone sweep");
    // G: quads per thread.  One; the arrays and loops over G are k_sweepc's form of the level body, kept (profiles/switch_retirement.md).
    constexpr int G = 1, NT = sweepz_nt(NQ), NG = 4 * G, NC = RRLW_SWEEPC_CODES, NVAL = IDRV ? 4 : 2;
    constexpr int NS2 = MODE == 2 ? NG : 1;          // rtrnmr's extra state
    constexpr int NSD = IDRV ? NG : 1;               // d/dT state
    extern __shared__ __align__(16) unsigned char smem[];
    // (a group without cloud is k_sweepc<., 0>'s - SweepArgs::cfree: the surface, all that is left for the zone there, is done by that launch)
    const int ltop = __builtin_amdgcn_readfirstlane(W.hgrp[(blockIdx.x * blockDim.z) / SORT_GROUP]);       // layers 1 .. ltop (uniform over the workgroup): one scalar load, before anything is staged
    if (a.cfree && ltop == 0) return;
    const int tx = threadIdx.x, ty = __builtin_amdgcn_readfirstlane(threadIdx.y), sub = __builtin_amdgcn_readfirstlane(threadIdx.z);
    const int bi = ty / NT, part = ty % NT;
    const int ny = blockDim.y, nb = ny / NT, nsb = blockDim.z, ncw = 64 * nsb;
    const float2 *s_lut = reinterpret_cast<const float2 *>(smem);
    double (*s_pl)[184] = reinterpret_cast<double (*)[184]>(smem + SWEEP_LUT_BYTES + bi * SWEEPC_BAND_BYTES);
    double (*s_fr)[16] = reinterpret_cast<double (*)[16]>(smem + SWEEP_LUT_BYTES + bi * SWEEPC_BAND_BYTES + SWEEP_PL_BYTES);
    double *red = reinterpret_cast<double *>(smem + SWEEP_LUT_BYTES + nb * SWEEPC_BAND_BYTES);      // [2][NVAL][ny][NC][ncw]
    const int cblock = __builtin_amdgcn_readfirstlane(W.order[blockIdx.x * nsb + sub]);       // the wave's 64-column block (see k_sweepc)
    const int col = cblock * 64 + tx;
    const int bsel = a.split ? (int)blockIdx.y : 0;                             // (see k_sweepc)
    const unsigned long long bands = a.bands >> (4 * bsel);
    const int B = (int)((bands >> (4 * bi)) & 15ull) + 1;
    const bool incol = col < a.ncol;
    const int colc = incol ? col : a.ncol - 1;
    const int quad = __builtin_amdgcn_readfirstlane(band_qstart(B) + part * G);
    const int g0 = NG * part;
    const int pc = pcol(W, colc);                                               // (see k_sweepc)
    const size_t gc = (size_t)a.col0 + pc;
    const int nlay = W.nlay, nct = a.nct;
    const size_t ncb = W.ncolb;
    const bool alt16 = (B == 16 && a.istart == 16);
    const bool lo_bin = (LO_BINARY >> (B - 1)) & 1u, up_bin = (UP_BINARY >> (B - 1)) & 1u;
    const bool any_bin = lo_bin || up_bin;
    const int base_up = ((UP_ZERO >> (B - 1)) & 1u) ? 14 : (((UP_FROM_A >> (B - 1)) & 1u) ? 0 : 9);
    sweep_stage_lut(T, smem, (sub * ny + ty) * 64 + tx, 64 * ny * nsb);
    sweep_stage_band(T, s_pl, s_fr, B, alt16, lo_bin, up_bin, (sub * NT + part) * 64 + tx, NT * ncw);
    __syncthreads();
    const size_t qstride = (size_t)nlay * ncb;
    const unsigned *__restrict__ sC = W.scr[S_CODE] + (size_t)quad * qstride * CODE_WORDS;
    const unsigned *__restrict__ sCt = W.scr[S_CODET] + (size_t)quad * qstride * CODE_WORDS;
    const unsigned *__restrict__ sFw = W.fw + (size_t)fw_slot(B) * nlay * ncb;
    const int *__restrict__ sFlag = W.cflag;
    const bool moved = pmoved(W, colc);                                         // (see k_sweepc)
    const double *__restrict__ tlay = moved ? W.tlayc : a.tlay + a.col0;
    const double *__restrict__ tlev = moved ? W.tlevc : a.tlev + a.col0;
    const double *__restrict__ cldf = moved ? W.cldfc : a.cldfrac + a.col0;
    const size_t tstride = moved ? ncb : (size_t)nct;
    const unsigned off16 = (unsigned)colc * 16u, offc = (unsigned)colc * (unsigned)CODE_BYTES, off8 = (unsigned)colc * 8u, off4 = (unsigned)colc * 4u;
    const size_t pcb = (size_t)W.pcb;
    const size_t gslab = (size_t)(a.group + bsel) * (nlay + 1) * pcb;
    Part2 *__restrict__ gdn = W.gdn + gslab;
    Part2 *__restrict__ gup = W.gup + gslab;
    Part2 *__restrict__ gdp = W.gdp + gslab;
    const unsigned so16 = (unsigned)col * 16u;
    const int laytrop = W.laytrop[colc];
    const double *tp0 = s_pl[0], *tp1 = s_pl[1];
    double2 *hand = reinterpret_cast<double2 *>(W.hand) + ((size_t)quad * ncb + colc) * 2;
    const size_t hstream = (size_t)NQUAD * ncb * 2;
    const bool colcloud = (bload_u32(sFlag, off4) & 8u) != 0;
    // MODE 4: the mask bits of this thread's g-points (bits of padding g-points cleared): first g-point, its words, valid count
    const int ig0 = band_g0(B) + g0, mw0 = ig0 >> 5, mw1 = mw0 < 4 ? mw0 + 1 : 4;
    const int nvalid = max(0, min(NG, band_ng(B) - g0));

    auto clampl = [&](int lev) { return min(max(lev, 1), nlay); };
    // the level's own inputs, one level ahead; zoff: 0 = interface below the layer (downward), 1 = above (upward)
    // (LITE: a level below the group's lowest cloud - no column of the workgroup is cloudy there: its cloud fraction and flag word are not read)
    const unsigned ncb32 = (unsigned)ncb, tstr32 = (unsigned)tstride;
    auto fill_t = [&](auto bin_tag, auto lite_tag, int lev, int zoff, SweepzLev &q) {
        const unsigned r = (unsigned)(clampl(lev) - 1);
        q.tl = bload_f64(row_ptr(tlay, r, tstr32), off8);
        q.tz = bload_f64(row_ptr(tlev, r + (unsigned)zoff, tstr32), off8);
        if constexpr (!decltype(lite_tag)::value) {
            q.cf = bload_f64(row_ptr(cldf, r, tstr32), off8);
            q.flag = bload_u32(sFlag, off4, (r + 1u) * ncb32 * 4u);
        }
        if constexpr (decltype(bin_tag)::value) q.w = bload_u32(sFw, off4, r * ncb32 * 4u);
    };
    auto ld_c = [&](const unsigned *base, int lev, int k) -> pk4 {
        return bload_pk4_nt(base + (size_t)k * qstride * CODE_WORDS, offc, (unsigned)(clampl(lev) - 1) * ncb32 * (unsigned)CODE_BYTES);
    };
    auto frac_row = [&](int lev, unsigned fwv, double &fpl) -> const double * {
        const bool lower = lev <= laytrop;
        if (any_bin) {          // uniform
            const unsigned w = (lower ? lo_bin : up_bin) ? fwv : 0x10000000u;
            const int r0 = clampi((lower ? 0 : base_up) + (int)(w >> 28) - 1, 0, 14);
            fpl = (double)(w & 0x0fffffffu) * (1.0 / 268435456.0);
            return &s_fr[r0][g0];
        }
        fpl = 0.0;
        return &s_fr[lower ? 0 : base_up][g0];
    };

    // reduction over the group, as in k_sweepc (raw sums in, band weight applied by the reducing wave)
    const unsigned rlane = (unsigned)(sub * 64 + tx);
    const unsigned vstride = (unsigned)(ny * NC * ncw), rband = (unsigned)(ty * NC * ncw);
    unsigned bufoff = 0u;
    auto red_put = [&](int c, int val, double v) { red[bufoff + val * vstride + rband + (unsigned)(c * ncw) + rlane] = v; };
    auto round_end = [&](auto dn_tag, int lev0, int nvalid) __attribute__((always_inline)) {
#pragma clang fp contract(off)      // (as in k_sweepc)
        constexpr bool DN = decltype(dn_tag)::value;
        __syncthreads();
        constexpr int NV = DN ? 2 : NVAL;
        for (int c = ty; c < nvalid; c += ny) {       // (wave-uniform)
            const int lvl = DN ? lev0 - c - 1 : lev0 + c;
            double sv[NV];
#pragma unroll
            for (int val = 0; val < NV; val++) {
                const double *r = red + (bufoff + val * vstride + (unsigned)(c * ncw) + rlane);
                double sum = 0.0;
                for (int q = 0; q < nb; q++) {
                    // (the band's quads in k_sweepc's order - pairs first: a level's partial must not depend on which of the two kernels swept it,
                    // i.e. on the hand-off level its block happened to get)
                    double pq = r[(unsigned)(q * NT * NC * ncw)];
                    if constexpr (NT >= 2) pq = pq + r[(unsigned)((q * NT + 1) * NC * ncw)];
                    if constexpr (NT == 3) pq = pq + r[(unsigned)((q * NT + 2) * NC * ncw)];
                    if constexpr (NT == 4) pq = pq + (r[(unsigned)((q * NT + 2) * NC * ncw)] + r[(unsigned)((q * NT + 3) * NC * ncw)]);
                    const int bq = (int)((bands >> (4 * q)) & 15ull);
                    double v = (pq * 0.5) * T.delwave[bq];
                    if (val >= 2) v = v * T.fluxfac;
                    sum = q == 0 ? v : sum + v;
                    if constexpr (SPEC) {
                        if (incol && val < 2) {             // (total, clear; not their d/dT)
                            double *dst = val == 0 ? (DN ? a.dflxs : a.uflxs) : (DN ? a.dflxcs : a.uflxcs);
                            if (dst) dst[spec_at(gc, lvl, bq + 1, nlay, nct)] = v * T.fluxfac;
                        }
                    }
                }
                sv[val] = sum;
            }
            if (incol) {
                bstore_f64x2((DN ? gdn : gup) + (size_t)lvl * pcb, so16, sv[0], sv[1]);
                if constexpr (IDRV && !DN) bstore_f64x2(gdp + (size_t)lvl * pcb, so16, sv[2], sv[3]);
            }
        }
        bufoff = bufoff ? 0u : NVAL * vstride;
    };

    // state: total-sky radiance, clear-sky radiance, rtrnmr's cloudy / clear parts and carried correction, per g-point
    double rad[NG], radc[NG], cldrad[NS2], clrrad[NS2], radmr[NS2], drad[NSD], dradc[NSD];
#pragma unroll
    for (int j = 0; j < NS2; j++) { cldrad[j] = 0.0; clrrad[j] = 0.0; radmr[j] = 0.0; }
    {                               // downward radiances at level ltop from k_sweepc<., 1>; clear = total up there
#pragma unroll
        for (int k = 0; k < G; k++) {
            const double2 h0 = hand[(size_t)k * ncb * 2], h1 = hand[(size_t)k * ncb * 2 + 1];
            rad[4 * k] = h0.x; rad[4 * k + 1] = h0.y; rad[4 * k + 2] = h1.x; rad[4 * k + 3] = h1.y;
        }
        if (ltop == nlay) {         // the zone reaches the top of the column: nothing comes down into it (rtrn :352 radld = 0); with the zone
#pragma unroll                      // kernel walking all levels (k_blocksort, force_top) no clear-sky launch has written the hand-off array
            for (int j = 0; j < NG; j++) rad[j] = 0.0;
            if (incol && ty == 0) bstore_f64(W.gdn1 + gslab + (size_t)nlay * pcb, (unsigned)col * 8u, 0.0);      // downward flux at the top level
            if constexpr (SPEC) {
                if (incol && part == 0) {
                    const size_t o = spec_at(gc, nlay, B, nlay, nct);
                    a.dflxs[o] = 0.0;
                    if (a.dflxcs) a.dflxcs[o] = 0.0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NG; j++) radc[j] = rad[j];
    }
    bool seen = false;              // downward: a cloud lies above (iclddn); upward: the column holds cloud (set before the upward sweep)

    SweepzLev cur;
    cur.w = 0u;
    // code slots: NC levels of the gas codes in flight, one of the total (gas + cloud) ones (a second slot of those put the rtrnmr
    // instantiations 3-5 registers over their 168: scratch reloads count in vmcnt and drain the prefetches)
    pk4 cc[G][NC], ct[G];
    // One level.  DN: downward (Planck difference towards the interface below, partial of level lev - 1, istcldd = flag bit 1), else
    // upward (istcld = bit 2).  The overlap factors of the level are requested first and used last.
    auto level = [&](auto bin_tag, auto dn_tag, int lev, int slot) __attribute__((always_inline)) {
        constexpr bool BIN = decltype(bin_tag)::value, DN = decltype(dn_tag)::value;
        constexpr int dir = DN ? -1 : 1;
        double2 f0 = make_double2(0., 0.), f1 = f0, f2 = f0;
        double efcl = 0.0;
        unsigned mlo = 0u, mhi = 0u;
        float4 cf4[G], ef4[G];
        if constexpr (MODE == 2) {
            const double2 *ov = W.ovl + (size_t)(DN ? 0 : nlay + 1) * 3 * ncb;            // (the direction's half: uniform, fixed)
            const unsigned so = (unsigned)clampl(lev) * 3u * ncb32 * 16u;
            f0 = bload_f64x2(ov, off16, so); f1 = bload_f64x2(ov, off16, so + ncb32 * 16u); f2 = bload_f64x2(ov, off16, so + ncb32 * 32u);
        } else {
            if constexpr (MODE != 3) efcl = bload_f64(W.efcl + (size_t)(B - 1) * nlay * ncb, off8, (unsigned)(clampl(lev) - 1) * ncb32 * 8u);
            if constexpr (MODE == 3) {              // cloud fraction (0 / 1) and effective emissivity per g-point: 8 floats per quad
#pragma unroll
                for (int k = 0; k < G; k++) {
                    const float *pc = W.cfef + (size_t)(quad + k) * nlay * ncb * 8;
                    const unsigned so = (unsigned)(clampl(lev) - 1) * ncb32 * 32u;
                    const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(sweep_rsrc(pc), (int)((unsigned)colc * 32u), (int)so, 0);
                    const u32x4 e = __builtin_amdgcn_raw_buffer_load_b128(sweep_rsrc(pc), (int)((unsigned)colc * 32u + 16u), (int)so, 0);
                    __builtin_memcpy(&cf4[k], &c, 16);
                    __builtin_memcpy(&ef4[k], &e, 16);
                }
            }
            if constexpr (MODE == 4) {              // the two mask words that can hold this thread's g-points
                const unsigned moff = (unsigned)(W.mask_col0 + gc) * 4u;
                const unsigned *mrow = W.mask + (size_t)(clampl(lev) - 1) * W.mask_stride;
                mlo = bload_u32(mrow + (size_t)mw0 * nlay * W.mask_stride, moff);
                mhi = bload_u32(mrow + (size_t)mw1 * nlay * W.mask_stride, moff);
            }
        }
        double fpl;
        const double *row = frac_row(lev, cur.w, fpl);
        const double blay = planck_at(tp0, tp0, cur.tl);
        const double dpl = planck_at(tp0, (DN && alt16 && lev == 1) ? tp1 : tp0, cur.tz) - blay;
        const bool cloudy = (cur.flag & 1u) != 0u;
        const bool first = (cur.flag & (DN ? 2u : 4u)) != 0u;
        const double cf = cur.cf;
        const bool anycld = __builtin_amdgcn_ballot_w64(cloudy) != 0ull;       // (wave-uniform)
        unsigned gbits = 0u;
        if constexpr (MODE == 4) gbits = (unsigned)((((unsigned long long)mlo | ((unsigned long long)mhi << 32)) >> (ig0 & 31)) & ((1ull << nvalid) - 1ull));
        fill_t(bin_tag, std::false_type{}, lev + dir, DN ? 0 : 1, cur);
        double qs[G], qsc[G];
#pragma unroll
        for (int k = 0; k < G; k++) {
            pk4 pk, pkt;
#pragma unroll
            for (int c = 0; c < NC; c++) if (c == slot) { pk = cc[k][c]; pkt = ct[k]; }
            const scr4 ck = unpack4(pk), ckt = unpack4(pkt);
            float2 e[4], et[4];
#pragma unroll
            for (int jj = 0; jj < 4; jj++) e[jj] = s_lut[code_index(ck.v[jj])];
            if (anycld) {
#pragma unroll
                for (int jj = 0; jj < 4; jj++) et[jj] = s_lut[min(code_index(ckt.v[jj]), (unsigned)NTBL)];
            }
            {
                const pk4 nx = ld_c(sC, lev + NC * dir, k), nxt = ld_c(sCt, lev + dir, k);
#pragma unroll
                for (int c = 0; c < NC; c++) if (c == slot) { cc[k][c] = nx; ct[k] = nxt; }
            }
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int j = 4 * k + jj;
                double atr, tfn;
                decode(ck.v[jj], e[jj], atr, tfn);
                double fr = row[j];
                if constexpr (BIN) fr = fma(fpl, row[16 + j] - fr, fr);
                const double bb = fr * fma(tfn, dpl, blay);
                // clear level: rtrnmr :617-627 / :705-716
                const double rad_s = fma(bb - rad[j], atr, rad[j]);
                const double updc = fma(bb - radc[j], atr, radc[j]);
                if (!anycld) {
                    rad[j] = rad_s;
                    radc[j] = seen ? updc : rad_s;
                    if constexpr (IDRV && !DN) {
                        const double tr = one_minus(atr);
                        drad[j] = times(drad[j], tr);
                        dradc[j] = seen ? times(dradc[j], tr) : drad[j];
                    }
                } else {
                    // cloudy level: rtrnmr :591-615 / :680-703, formed for every lane of the wave and selected
                    double atot, tftot;
                    decode(ckt.v[jj], et[jj], atot, tftot);
                    const double bbtot = fr * fma(tftot, dpl, blay);
                    const double gassrc = bb * atr;
                    double rad_c;
                    if constexpr (MODE == 2) {
                        double cr = cldrad[j], lr = clrrad[j], mr = radmr[j];
                        if (first) { cr = cf * rad[j]; lr = rad[j] - cr; mr = 0.0; }
                        const double ttot = one_minus(atot), tgas = one_minus(atr), clr = one_minus(cf);
                        const double cldsrc = bbtot * atot;
                        cr = fma(cr, ttot, cf * cldsrc);
                        lr = fma(lr, tgas, clr * gassrc);
                        rad_c = cr + lr;
                        const double radmod = fma(f1.y, cldsrc, fma(-f1.x, gassrc, mr * fma(f0.x, tgas, f0.y * ttot)));
                        const double oldcld = cr - radmod;
                        const double oldclr = lr + radmod;
                        mr = fma(-f2.y, oldcld, fma(f2.x, oldclr, -radmod));
                        // (the cloudy / clear parts and the carried correction of a lane that is clear at this level need not be kept:
                        // the next cloudy level of that column is the first of a block, istcld = 1, and sets them anew)
                        cldrad[j] = cr + mr;
                        clrrad[j] = lr - mr;
                        radmr[j] = mr;
                    } else {                        // rtrn :372-435 / rtrnmc: the same explicit fused form in both flavours (the array and the mask
                        double cfj = cf, efj = efcl;    // flavour of rtrnmc must round identically)
                        if constexpr (MODE == 4) { const bool on = (gbits >> j) & 1u; cfj = on ? 1.0 : 0.0; efj = on ? efcl : 0.0; }
                        if constexpr (MODE == 3) {
                            const float *c4 = reinterpret_cast<const float *>(&cf4[k]), *e4 = reinterpret_cast<const float *>(&ef4[k]);
                            cfj = c4[jj]; efj = e4[jj];
                        }
                        rad_c = fma(cfj, fma(bbtot, atot, -gassrc), fma(-rad[j], fma(efj, 1. - atr, atr), rad[j]) + gassrc);
                    }
                    rad[j] = cloudy ? rad_c : rad_s;
                    radc[j] = (cloudy || seen) ? updc : rad_s;
                    if constexpr (IDRV && !DN) {        // d/dT: rtrnmr :697-702 (cloudy), :712-714 (clear)
                        double cfd = cf;
                        if constexpr (MODE == 4) cfd = ((gbits >> j) & 1u) ? 1.0 : 0.0;
                        if constexpr (MODE == 3) cfd = reinterpret_cast<const float *>(&cf4[k])[jj];
                        const double tr = one_minus(atr);
                        const double d_s = times(drad[j], tr);
                        const double d_c = times(drad[j] * cfd, one_minus(atot)) + times(drad[j] * one_minus(cfd), tr);     // (rtrnmr :697-699: two products and their sum, rounded as written)
                        const double dc_s = seen ? times(dradc[j], tr) : d_s;
                        drad[j] = cloudy ? d_c : d_s;
                        dradc[j] = cloudy ? times(dradc[j], tr) : dc_s;
                    }
                }
            }
            qs[k] = (rad[4 * k] + rad[4 * k + 1]) + (rad[4 * k + 2] + rad[4 * k + 3]);
            qsc[k] = (radc[4 * k] + radc[4 * k + 1]) + (radc[4 * k + 2] + radc[4 * k + 3]);
        }
        if constexpr (DN) seen = seen || cloudy;
        red_put(slot, 0, qs[0]);
        red_put(slot, 1, qsc[0]);
        if constexpr (IDRV && !DN) {
            double ds = 0.0, dsc = 0.0;
#pragma unroll
            for (int k = 0; k < G; k++) {
                ds = ds + ((drad[4 * k] + drad[4 * k + 1]) + (drad[4 * k + 2] + drad[4 * k + 3]));
                dsc = dsc + ((dradc[4 * k] + dradc[4 * k + 1]) + (dradc[4 * k + 2] + dradc[4 * k + 3]));
            }
            red_put(slot, 2, ds);
            red_put(slot, 3, dsc);
        }
    };
    // The same level below the lowest cloud of the workgroup's blocks (layers 1 .. lbot - 1: clear in every column): the clear-sky update of
    // both streams - the arithmetic of the branch above that a wave without a cloudy lane takes, rtrnmr :617-627 / :705-716 - without the
    // cloudy level's inputs (total-optical-depth codes, cloud fraction, flag word, overlap factors / emissivity / mask words).
    auto level_lite = [&](auto bin_tag, auto dn_tag, int lev, int slot) __attribute__((always_inline)) {
        constexpr bool BIN = decltype(bin_tag)::value, DN = decltype(dn_tag)::value;
        constexpr int dir = DN ? -1 : 1;
        double fpl;
        const double *row = frac_row(lev, cur.w, fpl);
        const double blay = planck_at(tp0, tp0, cur.tl);
        const double dpl = planck_at(tp0, (DN && alt16 && lev == 1) ? tp1 : tp0, cur.tz) - blay;
        fill_t(bin_tag, std::true_type{}, lev + dir, DN ? 0 : 1, cur);
        double qs[G], qsc[G];
#pragma unroll
        for (int k = 0; k < G; k++) {
            pk4 pk;
#pragma unroll
            for (int c = 0; c < NC; c++) if (c == slot) pk = cc[k][c];
            const scr4 ck = unpack4(pk);
            float2 e[4];
#pragma unroll
            for (int jj = 0; jj < 4; jj++) e[jj] = s_lut[code_index(ck.v[jj])];
            {
                const pk4 nx = ld_c(sC, lev + NC * dir, k);
#pragma unroll
                for (int c = 0; c < NC; c++) if (c == slot) cc[k][c] = nx;
            }
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int j = 4 * k + jj;
                double atr, tfn;
                decode(ck.v[jj], e[jj], atr, tfn);
                double fr = row[j];
                if constexpr (BIN) fr = fma(fpl, row[16 + j] - fr, fr);
                const double bb = fr * fma(tfn, dpl, blay);
                const double rad_s = fma(bb - rad[j], atr, rad[j]);
                const double updc = fma(bb - radc[j], atr, radc[j]);
                rad[j] = rad_s;
                radc[j] = seen ? updc : rad_s;
                if constexpr (IDRV && !DN) {
                    const double tr = one_minus(atr);
                    drad[j] = times(drad[j], tr);
                    dradc[j] = seen ? times(dradc[j], tr) : drad[j];
                }
            }
            qs[k] = (rad[4 * k] + rad[4 * k + 1]) + (rad[4 * k + 2] + rad[4 * k + 3]);
            qsc[k] = (radc[4 * k] + radc[4 * k + 1]) + (radc[4 * k + 2] + radc[4 * k + 3]);
        }
        red_put(slot, 0, qs[0]);
        red_put(slot, 1, qsc[0]);
        if constexpr (IDRV && !DN) {
            double ds = 0.0, dsc = 0.0;
#pragma unroll
            for (int k = 0; k < G; k++) {
                ds = ds + ((drad[4 * k] + drad[4 * k + 1]) + (drad[4 * k + 2] + drad[4 * k + 3]));
                dsc = dsc + ((dradc[4 * k] + dradc[4 * k + 1]) + (dradc[4 * k + 2] + dradc[4 * k + 3]));
            }
            red_put(slot, 2, ds);
            red_put(slot, 3, dsc);
        }
    };
    // `count` levels from layer `first` in the sweep direction; LITE: the clear-sky levels below the lowest cloud
    auto sweep = [&](auto bin_tag, auto dn_tag, auto lite_tag, int first, int count) __attribute__((always_inline)) {
        constexpr bool DN = decltype(dn_tag)::value, LITE = decltype(lite_tag)::value;
        constexpr int dir = DN ? -1 : 1;
        if (count <= 0) return;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (c == NC - 1) fill_t(bin_tag, lite_tag, first, DN ? 0 : 1, cur);
#pragma unroll
            for (int k = 0; k < G; k++) {
                cc[k][c] = ld_c(sC, first + c * dir, k);
                if constexpr (!LITE) { if (c == 0) ct[k] = ld_c(sCt, first, k); }
            }
        }
        auto one = [&](int lev, int slot) __attribute__((always_inline)) {
            if constexpr (LITE) level_lite(bin_tag, dn_tag, lev, slot); else level(bin_tag, dn_tag, lev, slot);
        };
        int n = 0;
        for (; n + NC <= count; n += NC) {
#pragma unroll
            for (int c = 0; c < NC; c++) one(first + (n + c) * dir, c);
            round_end(dn_tag, first + n * dir, NC);
        }
        const int rem = count - n;
#pragma unroll
        for (int c = 0; c < NC - 1; c++) {
            if (c < rem) one(first + (n + c) * dir, c);
        }
        if (rem > 0) round_end(dn_tag, first + n * dir, rem);
    };
    using std::true_type;
    using std::false_type;
    // the zone in two parts: layers lbot .. ltop with the cloudy-level machinery, layers 1 .. lbot - 1 below every cloud of the workgroup
    const int lbot = ltop >= 1 ? min(max(__builtin_amdgcn_readfirstlane(W.hbot[(blockIdx.x * nsb) / SORT_GROUP]), 1), ltop) : 1;

    // ------------------------------------------------------------------ downward: layers ltop .. lbot, then lbot - 1 .. 1
    if (any_bin) { sweep(true_type{}, true_type{}, false_type{}, ltop, ltop - lbot + 1); sweep(true_type{}, true_type{}, true_type{}, lbot - 1, lbot - 1); }
    else { sweep(false_type{}, true_type{}, false_type{}, ltop, ltop - lbot + 1); sweep(false_type{}, true_type{}, true_type{}, lbot - 1, lbot - 1); }
    // ------------------------------------------------------------------ surface: rtrnmr :629-652
    {
        const double reflect = 1. - a.emis[gc + (size_t)nct * (B - 1)];
        const double pb = W.percol[(size_t)(PC_PLANKBND + B - 1) * ncb + colc];
        const double dpb = IDRV ? W.percol[(size_t)(PC_DPLANKBND + B - 1) * ncb + colc] : 0.0;
        double fpl;
        const double *row = frac_row(1, any_bin ? bload_u32(sFw, off4) : 0u, fpl);
        double usum = 0.0, usumc = 0.0, dusum = 0.0;
#pragma unroll
        for (int j = 0; j < NG; j++) {
            const double fr = any_bin ? fma(fpl, row[16 + j] - row[j], row[j]) : row[j];
            const double rad0 = fr * pb;
            rad[j] = fma(reflect, rad[j], rad0);
            radc[j] = fma(reflect, radc[j], rad0);
            usum = usum + rad[j];
            usumc = usumc + radc[j];
            if constexpr (MODE == 2) { cldrad[j] = 0.0; clrrad[j] = 0.0; radmr[j] = 0.0; }
            if constexpr (IDRV) { drad[j] = times(fr, dpb); dradc[j] = drad[j]; dusum = dusum + drad[j]; }
        }
        red_put(0, 0, usum);
        red_put(0, 1, usumc);
        if constexpr (IDRV) { red_put(0, 2, dusum); red_put(0, 3, dusum); }
        round_end(false_type{}, 0, 1);              // level 0
    }
    seen = colcloud;
    // ------------------------------------------------------------------ upward: layers 1 .. lbot - 1, then lbot .. ltop
    if (any_bin) { sweep(true_type{}, false_type{}, true_type{}, 1, lbot - 1); sweep(true_type{}, false_type{}, false_type{}, lbot, ltop - lbot + 1); }
    else { sweep(false_type{}, false_type{}, true_type{}, 1, lbot - 1); sweep(false_type{}, false_type{}, false_type{}, lbot, ltop - lbot + 1); }
    if (incol) {                    // upward radiances at level ltop for k_sweepc<., 2>
        // (the hand-off address is formed again from the lane's column offset, hidden from common-subexpression elimination: held in
        // registers from the first use at the top of the kernel it cost the rtrnmr instantiations the two registers they were over budget)
        unsigned o4 = off4;
        asm volatile("" : "+v"(o4));
        double2 *hand_up = reinterpret_cast<double2 *>(W.hand) + ((size_t)quad * ncb + (o4 >> 2)) * 2;
#pragma unroll
        for (int k = 0; k < G; k++) {
            double2 *h = hand_up + (size_t)k * ncb * 2;
            h[hstream] = make_double2(rad[4 * k], rad[4 * k + 1]);        h[hstream + 1] = make_double2(rad[4 * k + 2], rad[4 * k + 3]);
            h[2 * hstream] = make_double2(radc[4 * k], radc[4 * k + 1]);  h[2 * hstream + 1] = make_double2(radc[4 * k + 2], radc[4 * k + 3]);
            if constexpr (IDRV) {
                h[3 * hstream] = make_double2(drad[4 * k], drad[4 * k + 1]);    h[3 * hstream + 1] = make_double2(drad[4 * k + 2], drad[4 * k + 3]);
                h[4 * hstream] = make_double2(dradc[4 * k], dradc[4 * k + 1]);  h[4 * hstream + 1] = make_double2(dradc[4 * k + 2], dradc[4 * k + 3]);
            }
        }
    }
}

#pragma clang fp contract(fast)
// ------------------------------------------------------------------------------------------------
// k_n1 : PROTOTYPE of the mapping BASELINE.json's north_star names, for cloud-free calls (icld = 0), kept to put a number beside the
//        production mapping ("north-star mapping"): ONE COLUMN PER WAVEFRONT, G-POINTS ACROSS LANES (three passes over the
//        152 padded g-slots), Planck / fraction tables in LDS, the transmittance either from the table in LDS or (EXPF) from
//        __builtin_amdgcn_exp2f, WAVE-REDUCE of the g-point radiances: the reduction covers all 16 bands at once, so the wave writes
//        the column's FINAL fluxes and heating rates - no per-band partial slabs, no k_flux / k_rates.  It reads k_layer's codes.
//        Per level the wave does what k_sweepc does once per 64 columns: 16 Planck pairs (one lane per band), the fraction rows, and a
//        64-lane reduction - which is why it loses (measured: profiles/round2_n1.md).
// ------------------------------------------------------------------------------------------------
constexpr int N1_WAVES = 8;                                   // columns per workgroup
constexpr int N1_PL_BYTES = 16 * 184 * 8, N1_FR_BYTES = 16 * 16 * 16 * 8;
constexpr int N1_WAVE_BYTES = 16 * 32 + 2 * 608;              // per wave: {blay, dpl, fpl, row} per band; up / down flux per level (<= 603 layers: see n1_max_nlay)
__host__ __device__ constexpr int n1_lds_bytes(int nlay) { return SWEEP_LUT_BYTES + N1_PL_BYTES + N1_FR_BYTES + N1_WAVES * (16 * 32 + 2 * 8 * (nlay + 1)); }

template <bool IDRV_UNUSED>
__global__ __launch_bounds__(64 * N1_WAVES) void k_n1(DevTables T, Workspace W, SweepArgs a, FluxOut out, const double *pz)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const float2 *s_lut = reinterpret_cast<const float2 *>(smem);
    double (*s_pl)[184] = reinterpret_cast<double (*)[184]>(smem + SWEEP_LUT_BYTES);                          // [band][181]
    double (*s_fr)[16][16] = reinterpret_cast<double (*)[16][16]>(smem + SWEEP_LUT_BYTES + N1_PL_BYTES);    // [band][row][g]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nlay = W.nlay, nct = a.nct;
    const size_t ncb = W.ncolb;
    unsigned char *wbase = smem + SWEEP_LUT_BYTES + N1_PL_BYTES + N1_FR_BYTES + (size_t)wv * (16 * 32 + 2 * 8 * (nlay + 1));
    double *s_pk = reinterpret_cast<double *>(wbase);                    // [band][4]: blay, dpl, fpl, (row index as double)
    double *s_dn = reinterpret_cast<double *>(wbase + 16 * 32), *s_up = s_dn + (nlay + 1);
    {   // stage: transmittance table, every band's Planck row and fraction rows
        const int tid = threadIdx.x, nth = 64 * N1_WAVES;
        const double2 *src = reinterpret_cast<const double2 *>(T.stat + T.sl.lutf);
        double2 *dst = reinterpret_cast<double2 *>(smem);
        for (int i = tid; i < SWEEP_LUT_BYTES / 16; i += nth) dst[i] = src[i];
        for (int i = tid; i < 16 * 181; i += nth) s_pl[i / 181][i % 181] = T.stat[T.sl.totplnk + i];
        for (int i = tid; i < 16 * 16 * 16; i += nth) {
            const int b = i >> 8, r = (i >> 4) & 15, g = i & 15;
            const bool lo_bin = (LO_BINARY >> b) & 1u, up_bin = (UP_BINARY >> b) & 1u;
            const int ng = T.band[b].ng, fa = T.band[b].fracrefa, fb = T.band[b].fracrefb;
            const int na = lo_bin ? 9 : 1, nb = up_bin ? 5 : 1;
            double v = 0.0;
            if (g < ng) {
                if (r < 9) { if (r < na) v = T.ktab[fa + r * ng + g]; }
                else if (r < 14 && fb >= 0 && r - 9 < nb) v = T.ktab[fb + (r - 9) * ng + g];
            }
            s_fr[b][r][g] = v;
        }
        __syncthreads();
    }
    const int col = blockIdx.x * N1_WAVES + wv;
    if (col >= a.ncol) return;                      // (whole wave; no barrier follows)
    const size_t gc = (size_t)a.col0 + col;
    const int laytrop = W.laytrop[col];
    // lane -> g-slot of each pass: slot = 64 p + lane of the 152 padded slots (38 quads x 4)
    constexpr int NP1 = (4 * NQUAD + 63) / 64;       // passes over the padded g-slots (3 for 152, 4 for 256)
    int bnd[NP1], gi[NP1];
    double wt[NP1];
    size_t coff[NP1];
    bool ok[NP1];
#pragma unroll
    for (int p = 0; p < NP1; p++) {
        const int slot = 64 * p + lane, q = slot >> 2;
        int b = 0;
#pragma unroll
        for (int B = 1; B <= NBND; B++) if (q >= band_qstart(B)) b = B - 1;
        bnd[p] = b;
        gi[p] = 4 * (q - band_qstart(b + 1)) + (slot & 3);
        ok[p] = slot < 4 * NQUAD && gi[p] < T.band[b].ng;
        gi[p] = min(gi[p], 15);
        wt[p] = ok[p] ? 0.5 * T.delwave[b] : 0.0;
        coff[p] = ((size_t)min(q, NQUAD - 1) * nlay * ncb + col) * 4 + (slot & 3);        // + (lev - 1) * ncb * 4
    }
    const scr_t *codes = reinterpret_cast<const scr_t *>(W.scr[S_CODE]);      // (the prototype reads 32-bit codes: rrtmg_lw_hip_set_n1_prototype refuses other builds)
    // per level: lanes 0..15 (band = lane & 15) publish the band's Planck terms and fraction row
    const int mb = lane & 15;
    const bool m_lo_bin = (LO_BINARY >> mb) & 1u, m_up_bin = (UP_BINARY >> mb) & 1u;
    const int m_base_up = ((UP_ZERO >> mb) & 1u) ? 14 : (((UP_FROM_A >> mb) & 1u) ? 0 : 9);
    const int m_fwslot = fw_slot(mb + 1);
    auto publish = [&](int lev, int zlev, bool alt) {
        const double tl = a.tlay[gc + (size_t)nct * (lev - 1)], tz = a.tlev[gc + (size_t)nct * zlev];
        const bool lower = lev <= laytrop;
        unsigned w = 0x10000000u;
        if (lower ? m_lo_bin : m_up_bin) w = W.fw[((size_t)m_fwslot * nlay + (lev - 1)) * ncb + col];
        const int r0 = clampi((lower ? 0 : m_base_up) + (int)(w >> 28) - 1, 0, 14);
        const double fpl = (double)(w & 0x0fffffffu) * (1.0 / 268435456.0);
        const double *tp = s_pl[mb];
        const double blay = planck_at(tp, tp, tl);
        const double *tq = (alt && mb == 15) ? T.stat + T.sl.totplk16 : tp;        // (istart = 16 is not routed here; kept for symmetry)
        const double dpl = planck_at(tp, tq, tz) - blay;
        __builtin_amdgcn_wave_barrier();          // (the level before has read its entries)
        if (lane < 16) { s_pk[4 * mb] = blay; s_pk[4 * mb + 1] = dpl; s_pk[4 * mb + 2] = fpl; s_pk[4 * mb + 3] = (double)r0; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto wave_sum = [&](double v) -> double {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
    double rad[NP1];
#pragma unroll
    for (int p = 0; p < NP1; p++) rad[p] = 0.0;
    auto level = [&](int lev) -> double {
        double part = 0.0;
#pragma unroll
        for (int p = 0; p < NP1; p++) {
            const scr_t cj = ok[p] ? codes[coff[p] + (size_t)(lev - 1) * ncb * 4] : (scr_t)0;
            double atr, tfn;
            decode(cj, s_lut[code_index(cj)], atr, tfn);
            const int b = bnd[p];
            const double blay = s_pk[4 * b], dpl = s_pk[4 * b + 1], fpl = s_pk[4 * b + 2];
            const int r0 = (int)s_pk[4 * b + 3];
            const double f0 = s_fr[b][r0][gi[p]], f1 = s_fr[b][r0 + 1][gi[p]];
            const double fr = f0 + fpl * (f1 - f0);
            const double bb = fr * (blay + tfn * dpl);
            rad[p] = rad[p] + (bb - rad[p]) * atr;
            part += wt[p] * rad[p];
        }
        return wave_sum(part);
    };
    // ---- downward
    if (lane == 0) s_dn[nlay] = 0.0;
    for (int lev = nlay; lev >= 1; lev--) {
        publish(lev, lev - 1, false);
        const double f = level(lev);
        if (lane == 0) s_dn[lev - 1] = f * T.fluxfac;
    }
    // ---- surface
    {
        publish(1, 0, false);          // fraction row of layer 1
        double part = 0.0;
#pragma unroll
        for (int p = 0; p < NP1; p++) {
            const int b = bnd[p];
            const double fpl = s_pk[4 * b + 2];
            const int r0 = (int)s_pk[4 * b + 3];
            const double f0 = s_fr[b][r0][gi[p]], f1 = s_fr[b][r0 + 1][gi[p]];
            const double fr = f0 + fpl * (f1 - f0);
            const double reflect = 1. - a.emis[gc + (size_t)nct * b];
            const double pb = W.percol[(size_t)(PC_PLANKBND + b) * ncb + col];
            rad[p] = fr * pb + reflect * rad[p];
            part += wt[p] * rad[p];
        }
        const double f = wave_sum(part);
        if (lane == 0) s_up[0] = f * T.fluxfac;
    }
    // ---- upward
    for (int lev = 1; lev <= nlay; lev++) {
        publish(lev, lev, false);
        const double f = level(lev);
        if (lane == 0) s_up[lev] = f * T.fluxfac;
    }
    // ---- outputs: lanes = levels
    for (int l0 = 0; l0 <= nlay; l0 += 64) {
        const int lev = l0 + lane;
        if (lev <= nlay) {
            const size_t o = gc + (size_t)nct * lev;
            const double u = s_up[lev], d = s_dn[lev];
            out.uflx[o] = u; out.dflx[o] = d; out.uflxc[o] = u; out.dflxc[o] = d;
            if (out.fnet) { out.fnet[o] = u - d; out.fnetc[o] = u - d; }
            if (lev < nlay) {
                const double h = T.heatfac * ((u - d) - (s_up[lev + 1] - s_dn[lev + 1])) / (pz[o] - pz[o + nct]);
                out.hr[o] = h; out.hrc[o] = h;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_flux  : sum of the group partials (rtrn :549-574), flux scaling (rtrn :580-594), net flux and heating rate (rtrn :583-604; output
//           copies src/rrtmg_lw_rad.nomcica.f90:563-583).  A workgroup covers a WINDOW of 256 positions and a CHUNK of FLUX_CH
//           consecutive levels.  A thread owns one position and walks the chunk's levels upward with the net fluxes u - d, uc - dc and
//           the pressure of the level below in registers (the form k_adjust_cf has), so the heating rate of a layer needs no second
//           look at a level; a chunk that does not start at the surface sums the level below its first one once more - the level
//           belongs to the chunk before, which stores it.  The usual case - four groups of one slab each - has a straight-line body:
//           the loads of level k + 1 are issued before the sums of level k are used.  Any other group list (SweepArgs::split: a slab
//           per band; fewer groups) takes the loop over groups and slabs.
//           The partials lie by POSITION, the caller's arrays by COLUMN (k_colsort).  In a window that kept its order (wsort == 0, or
//           no order at all) position = column and the thread stores what it summed, straight from registers.  In a reordered window
//           the values of a level change places through a double-buffered LDS tile - position -> column, one barrier per level - and
//           thread t writes column w0 + t of the caller's arrays and reads its pressure: loads and stores stay coalesced either way.
//           (Gathered at the column's position, eight bytes per lane, the slabs cost a third more - sixteen cache lines per access
//           instead of four -, scattered to the position's column the outputs 60 %.)  The branch is uniform over the workgroup.
//           clear_from_total: a cloud-free call, the clear-sky stream equals the total-sky stream.  clear_groups: so it does in the
//           cloud-free block groups of a cloudy call, whose clear-sky sums are formed here from copies of the total ones - the values
//           k_sweepc<., 2> wrote twice before.  Only bands in [istart, iend] were
//           swept: the groups hold exactly those.
//           The sums keep their order - a group's slabs first, in list order, then the groups in order, then x fluxfac - and the
//           heating rate its expression, so the results are those of the kernel's earlier forms bit for bit.
// ------------------------------------------------------------------------------------------------
constexpr int FLUX_CH = 18;                     // levels of a chunk: 73 levels are 4 chunks and one of a single level; 250 000 columns 19 workgroups per CU
constexpr int FLUX_NG = 4;                      // groups of the straight-line body, one slab each
constexpr unsigned long long FLUX_GSZ1 = 0x1111ull;        // ... as `gsz` states them
template <bool IDRV> struct FluxRaw { Part2 u[FLUX_NG], d[FLUX_NG], q[IDRV ? FLUX_NG : 1]; };      // a level's group partials as loaded
struct FluxVal { double u, d, uc, dc, du, duc; };
constexpr int flux_lds_bytes(bool idrv) { return 2 * (idrv ? 6 : 4) * COLSORT_WIN * 8; }           // the exchange tile: 16 KB, 24 KB with d/dT
// A call that averages several sub-column samples (rrtmg_lw_hip_run_mcica_samples) runs the solver once per sample; k_flux of sample 0
// stores (ACC = 0, as in every other call), that of a later sample adds its total-sky values to what the caller's arrays hold (ACC = 1),
// that of the last one adds and divides by the number of samples (ACC = 2): the float64 sum in sample order and one division, no pass
// of its own over the outputs.  The clear-sky outputs do not depend on the sample: sample 0 has stored them.
template <int ACC>
__device__ __forceinline__ void flux_put(double *p, double x, double nsamp)
{
#pragma clang fp contract(off)      // (the sample's value rounds before it is added, as the stored value of a single call has)
    if constexpr (ACC == 0) *p = x;
    else if constexpr (ACC == 1) *p = *p + x;
    else *p = (*p + x) / nsamp;
}
// The statistics flavour (STAT, k_flux_var): beside the sum S in the mean's array a second sum M in the variance's array, both formed
// where the sample's value is - no array, pass or workspace of its own.  x: the value a single call would store for this sample,
// cnt = s + 1 for sample s.  Sample 0 stores S = x, M = 0; sample s >= 1
//     S = S + x,   t = cnt x - S  (the product rounds, then the difference),   M = M + t t / (cnt (cnt - 1))
// (Welford's update of the sum of squared deviations written on the running sum: cnt x - S = cnt (x - mean_cnt), and cnt (cnt - 1) is
// exact); the last sample leaves mean = S / nsamp - the bits of flux_put<2> - and var = M / (nsamp - 1), the unbiased sample variance.
// v may be null: the mean alone.
template <int ACC>
__device__ __forceinline__ void flux_stat(double *p, double *v, double x, double cnt, double nsamp)
{
#pragma clang fp contract(off)      // (every product and quotient rounds on its own: the recurrence is stated operation by operation)
    if constexpr (ACC == 0) { *p = x; if (v) *v = 0.0; }
    else {
        const double S = *p + x;
        if constexpr (ACC == 1) *p = S; else *p = S / nsamp;
        if (v) {
            const double tc = cnt * x;
            const double t = tc - S;
            const double tt = t * t;
            const double M = *v + tt / (cnt * (cnt - 1.0));
            if constexpr (ACC == 1) *v = M; else *v = M / (nsamp - 1.0);
        }
    }
}
template <bool IDRV, int ACC, bool STAT = false>
__device__ __forceinline__ void flux_body(const DevTables &T, const Workspace &W, const FluxOut &out, const double *pz, int ncol, int col0, int nct,
                                          int clear_from_total, int ngroups, unsigned long long gsz, int clear_groups, double nsamp, double cnt = 1.0)
{   // gsz: slabs per group, a nibble each (1, or - SweepArgs::split - the group's bands: added first, in their order, like the group's workgroup does)
    constexpr int NV = IDRV ? 6 : 4;                        // values of a level that change places
    __shared__ double s_v[2][NV][COLSORT_WIN];
    static_assert(sizeof(s_v) == flux_lds_bytes(IDRV), "k_flux: the exchange tile");
    const int t = threadIdx.x, w0 = blockIdx.x * COLSORT_WIN;
    const int slot = w0 + t;                                // the position whose partials this thread sums, and the column it writes
    const bool on = slot < ncol;
    const int nlay = W.nlay;
    const int k0 = blockIdx.y * FLUX_CH, k1 = min(nlay, k0 + FLUX_CH - 1), kf = max(k0 - 1, 0);       // the chunk's levels; the level the walk starts from
    const size_t gc = (size_t)col0 + slot;
    const bool moved = pmoved(W, w0);                       // (uniform over the workgroup)
    const int dst = (moved && on) ? W.perm[slot] - w0 : t;  // where the position's column lies in the window
    // Partials arrive summed per group of bands.  Downward at and above the hand-off level of the position's 64-column block, and everywhere
    // in a cloud-free call, the clear-sky stream equals the total one and one value was written (k_sweepc); below, and upward, two.
    // (uniform over the wave, and read as such: a wave's first lane is a column wherever any of its lanes is)
    const int ltop = __builtin_amdgcn_readfirstlane((on && !clear_from_total) ? W.hblk[slot >> 6] : 0);
    // (clear_groups - SweepArgs::cfree: a block whose hand-off level is 0 was swept by k_sweepc<., 0>, one value upward as well)
    const bool up1 = clear_from_total != 0 || (clear_groups != 0 && ltop == 0);
    const size_t pcb = (size_t)W.pcb, nlev = (size_t)nlay + 1;
    // the straight-line body's loads of one level: every group's slab, 8 or 16 bytes by the block's hand-off level
    const auto load = [&](int lev, FluxRaw<IDRV> &r) {
        if (!on) return;
        const size_t g0 = (size_t)lev * pcb + slot, gs = nlev * pcb;
        if (clear_from_total || lev >= ltop) {
#pragma unroll
            for (int g = 0; g < FLUX_NG; g++) { r.d[g].a = W.gdn1[g0 + g * gs]; r.d[g].b = r.d[g].a; }
        } else {
#pragma unroll
            for (int g = 0; g < FLUX_NG; g++) r.d[g] = W.gdn[g0 + g * gs];
        }
        if (up1) {
#pragma unroll
            for (int g = 0; g < FLUX_NG; g++) { r.u[g].a = W.gup1[g0 + g * gs]; r.u[g].b = r.u[g].a; }
        } else {
#pragma unroll
            for (int g = 0; g < FLUX_NG; g++) r.u[g] = W.gup[g0 + g * gs];
        }
        if constexpr (IDRV) {
#pragma unroll
            for (int g = 0; g < FLUX_NG; g++) r.q[g] = W.gdp[g0 + g * gs];
        }
    };
    // ... and their sums, the groups in order
    const auto sum = [&](const FluxRaw<IDRV> &r) -> FluxVal {
        double u = 0.0, d = 0.0, uc = 0.0, dc = 0.0, du = 0.0, duc = 0.0;
#pragma unroll
        for (int g = 0; g < FLUX_NG; g++) {
            u = u + r.u[g].a; uc = uc + r.u[g].b;
            d = d + r.d[g].a; dc = dc + r.d[g].b;
            if constexpr (IDRV) { du = du + r.q[g].a; duc = duc + r.q[g].b; }
        }
        return FluxVal{u, d, uc, dc, du, duc};
    };
    // any group list: the slabs of a group first, in list order, then the groups in order
    const auto sum_list = [&](int lev) -> FluxVal {
        double u = 0.0, d = 0.0, uc = 0.0, dc = 0.0, du = 0.0, duc = 0.0;
        if (on) {
            const bool dn1 = clear_from_total || lev >= ltop;
            int slab = 0;
            for (int g = 0; g < ngroups; g++) {
                const int n = (int)((gsz >> (4 * g)) & 15ull);
                Part2 su{0.0, 0.0}, sd{0.0, 0.0}, sq{0.0, 0.0};
                for (int q = 0; q < n; q++, slab++) {
                    const size_t go = ((size_t)slab * nlev + lev) * pcb + slot;
                    Part2 tu, td, tq{0.0, 0.0};
                    if (dn1) { td.a = W.gdn1[go]; td.b = td.a; } else td = W.gdn[go];
                    if (up1) { tu.a = W.gup1[go]; tu.b = tu.a; } else tu = W.gup[go];
                    if constexpr (IDRV) tq = W.gdp[go];
                    if (q == 0) { su = tu; sd = td; sq = tq; }
                    else { su.a = su.a + tu.a; su.b = su.b + tu.b; sd.a = sd.a + td.a; sd.b = sd.b + td.b; sq.a = sq.a + tq.a; sq.b = sq.b + tq.b; }
                }
                u = u + su.a; uc = uc + su.b;
                d = d + sd.a; dc = dc + sd.b;
                du = du + sq.a; duc = duc + sq.b;
            }
        }
        return FluxVal{u, d, uc, dc, du, duc};
    };
    double pb = 0.0, nb = 0.0, nbc = 0.0;                   // pressure and net fluxes of the level below
    // one level of the walk: scaling, the exchange where the window's columns moved, the column's stores
    const auto level = [&](int lev, FluxVal v, double p) {
        double u = v.u * T.fluxfac, d = v.d * T.fluxfac, uc, dc, du = v.du, duc = v.duc;
        if (clear_from_total) { uc = u; dc = d; duc = du; }
        else { uc = v.uc * T.fluxfac; dc = v.dc * T.fluxfac; }
        if (moved) {
            double (*s)[COLSORT_WIN] = s_v[lev & 1];        // (two tiles: a level's is read before the barrier of the next one, written again after it)
            s[0][dst] = u; s[1][dst] = d; s[2][dst] = uc; s[3][dst] = dc;
            if constexpr (IDRV) { s[4][dst] = du; s[5][dst] = duc; }
            __syncthreads();
            u = s[0][t]; d = s[1][t]; uc = s[2][t]; dc = s[3][t];
            if constexpr (IDRV) { du = s[4][t]; duc = s[5][t]; }
        }
        if (!on) return;
        const size_t o = gc + (size_t)nct * lev;
        const double net = u - d, netc = uc - dc;
        if (lev >= k0) {
            if constexpr (ACC == 0) {
                out.uflx[o] = u; out.dflx[o] = d; out.uflxc[o] = uc; out.dflxc[o] = dc;
                if (out.fnet) { out.fnet[o] = u - d; out.fnetc[o] = uc - dc; }
                if constexpr (IDRV) { out.duflx_dt[o] = du; out.duflxc_dt[o] = duc; }
                if constexpr (STAT) { if (out.uflx_var) out.uflx_var[o] = 0.0; if (out.dflx_var) out.dflx_var[o] = 0.0; }
            } else if constexpr (STAT) {
                flux_stat<ACC>(out.uflx + o, out.uflx_var ? out.uflx_var + o : nullptr, u, cnt, nsamp);
                flux_stat<ACC>(out.dflx + o, out.dflx_var ? out.dflx_var + o : nullptr, d, cnt, nsamp);
                if constexpr (IDRV) flux_put<ACC>(out.duflx_dt + o, du, nsamp);
            } else {
                flux_put<ACC>(out.uflx + o, u, nsamp); flux_put<ACC>(out.dflx + o, d, nsamp);
                if constexpr (IDRV) flux_put<ACC>(out.duflx_dt + o, du, nsamp);
            }
        }
        if (lev > kf) {             // net flux and heating rate of the layer below the level
            const double dp = pb - p;
            if constexpr (ACC == 0) {
                out.hr[o - (size_t)nct] = T.heatfac * (nb - net) / dp;
                out.hrc[o - (size_t)nct] = T.heatfac * (nbc - netc) / dp;
                if constexpr (STAT) { if (out.hr_var) out.hr_var[o - (size_t)nct] = 0.0; }
            } else if constexpr (STAT) flux_stat<ACC>(out.hr + (o - (size_t)nct), out.hr_var ? out.hr_var + (o - (size_t)nct) : nullptr, T.heatfac * (nb - net) / dp, cnt, nsamp);
            else flux_put<ACC>(out.hr + (o - (size_t)nct), T.heatfac * (nb - net) / dp, nsamp);
        }
        pb = p; nb = net; nbc = netc;
    };
    const double *const pzc = pz + gc;
    double p = on ? pzc[(size_t)nct * kf] : 0.0;
    if (ngroups == FLUX_NG && gsz == FLUX_GSZ1) {
        FluxRaw<IDRV> cur{}, nxt{};
        load(kf, cur);
        for (int lev = kf; lev <= k1; lev++) {
            double pn = 0.0;
            if (lev < k1) { load(lev + 1, nxt); if (on) pn = pzc[(size_t)nct * (lev + 1)]; }
            level(lev, sum(cur), p);
            cur = nxt; p = pn;
        }
    } else {
        for (int lev = kf; lev <= k1; lev++) {
            level(lev, sum_list(lev), p);
            if (lev < k1 && on) p = pzc[(size_t)nct * (lev + 1)];
        }
    }
}
template <bool IDRV>
__global__ __launch_bounds__(COLSORT_WIN) void k_flux(DevTables T, Workspace W, FluxOut out, const double *pz, int ncol, int col0, int nct,
                                                      int clear_from_total, int ngroups, unsigned long long gsz, int clear_groups)
{
    flux_body<IDRV, 0>(T, W, out, pz, ncol, col0, nct, clear_from_total, ngroups, gsz, clear_groups, 1.0);
}
// ... of sample 1 .. nsamp-1 of a call that averages samples (LAST: the one that divides)
template <bool IDRV, bool LAST>
__global__ __launch_bounds__(COLSORT_WIN) void k_flux_acc(DevTables T, Workspace W, FluxOut out, const double *pz, int ncol, int col0, int nct,
                                                          int clear_from_total, int ngroups, unsigned long long gsz, int clear_groups, double nsamp)
{
    flux_body<IDRV, LAST ? 2 : 1>(T, W, out, pz, ncol, col0, nct, clear_from_total, ngroups, gsz, clear_groups, nsamp);
}
// ... of a call that also wants the sample variances (FluxOut::uflx_var, dflx_var, hr_var): sample 0 (ACC = 0) stores and zeroes them,
// sample cnt - 1 adds (1), the last one adds and divides (2)
template <bool IDRV, int ACC>
__global__ __launch_bounds__(COLSORT_WIN) void k_flux_var(DevTables T, Workspace W, FluxOut out, const double *pz, int ncol, int col0, int nct,
                                                          int clear_from_total, int ngroups, unsigned long long gsz, int clear_groups, double nsamp, double cnt)
{
    flux_body<IDRV, ACC, true>(T, W, out, pz, ncol, col0, nct, clear_from_total, ngroups, gsz, clear_groups, nsamp, cnt);
}

// ------------------------------------------------------------------------------------------------
// k_calibrate : reads n 16-byte words per array with 16 B per lane and writes them back (known byte counts),
//               launched by rrtmg_lw_hip_calibrate_stream so that a PMC run can check the unit and scale of
//               FETCH_SIZE / WRITE_SIZE on this chip (MI355X_MICROARCH.md, HBM section) in the same session.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_calibrate(const double2 *__restrict__ in, double2 *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { double2 v = in[i]; v.x += 1.0; out[i] = v; }
}

// ------------------------------------------------------------------------------------------------
// k_adjust_cf / k_adjust_lf : rrtmg_lw_hip_adjust_tsfc* - the column driver's idrv = 1 adjustment (src/rrtmg_lw.1col.f90:587-605) of
//               the upward fluxes and heating rates of a stored radiation call to a changed surface temperature:
//                   u'(k) = uflx(k) + duflx_dt(k) * dtsfc        (multiply rounded, add rounded: never fused - adjust_up)
//                   hr(l) = heatfac * ((u'(l) - dflx(l)) - (u'(l+1) - dflx(l+1))) / (plev(l) - plev(l+1))       - k_flux's expression
//               in float64 on float64 or widened float32 arrays, total sky and (NS = 2) clear sky.  Nothing but traffic - 6.4 KB per
//               72-layer column -, so the kernels read and write the caller's arrays where they lie, in the caller's form (R: element
//               type, TOP: vertical index 0 at the top of the atmosphere), every element once, lanes along the form's fastest index.
//   k_adjust_cf   columns fastest, rows a.ld columns apart.  A thread owns V consecutive columns (V x sizeof(R) = 16 bytes per access where
//               every row of every array is 16-byte aligned - the first one is and both ncol and ld are multiples of V -, V = 1 otherwise) and walks the levels of its chunk (blockIdx.y) upward with the net flux and
//               pressure of the level below in registers.  A chunk reads the level it ends at once more; the level belongs to the next
//               chunk, which stores its u'.  The chunks only spread a small call over the chip: a large one walks whole columns.
//   k_adjust_lf   levels fastest: the (ncol, nlay+1) arrays are walked as ONE run of ncol x (nlay+1) values, V per thread, whatever
//               nlay + 1 is, so that every wave moves whole kilobytes.  The level above a thread's last value (below its first one
//               with TOP) is the next thread's: a second, scalar load that hits L1.  hr is (ncol, nlay): its values lie at other
//               offsets than the levels' - the run index minus the column (minus one with TOP) - and are stored one by one.
// ------------------------------------------------------------------------------------------------
struct AdjustSet { const void *u, *d, *du; void *ua, *hr; };
struct AdjustArgs {
    const void *plev, *dtsfc;
    AdjustSet s[2];             // total sky, clear sky
    unsigned long long ncol;    // columns of the call
    unsigned long long ld;      // k_adjust_cf: columns between two rows of the arrays (ncol, or the wider field's of a *_view call)
    int nlay, chunk;            // chunk: layers per blockIdx.y (k_adjust_cf)
    int vec;                    // k_adjust_lf: every level array starts on a 16-byte boundary
    double heatfac;
};
template <class R, int V> struct AdjustVec { typedef R type __attribute__((ext_vector_type(V))); };
// V values from p[at]: one access of V x sizeof(R) bytes (the caller has checked the alignment), or one value
template <class R, int V>
__device__ __forceinline__ void adjust_load(const void *p, size_t at, double (&x)[V])
{
    if constexpr (V == 1) x[0] = (double)static_cast<const R *>(p)[at];
    else {
        const typename AdjustVec<R, V>::type v = *reinterpret_cast<const typename AdjustVec<R, V>::type *>(static_cast<const R *>(p) + at);
#pragma unroll
        for (int j = 0; j < V; j++) x[j] = (double)v[j];
    }
}
template <class R, int V>
__device__ __forceinline__ void adjust_store(void *p, size_t at, const double (&x)[V])
{
    if constexpr (V == 1) static_cast<R *>(p)[at] = (R)x[0];
    else {
        typename AdjustVec<R, V>::type v;
#pragma unroll
        for (int j = 0; j < V; j++) v[j] = (R)x[j];
        *reinterpret_cast<typename AdjustVec<R, V>::type *>(static_cast<R *>(p) + at) = v;
    }
}
// u + du * dt with the product rounded before the sum.  Plain * and + under a contract-off pragma: __dmul_rn / __dadd_rn are inline
// functions in this compiler's headers whose operations carry the build's contract flag, and the two were fused into one v_fma_f64.
__device__ __forceinline__ double adjust_up(double u, double du, double dt)
{
#pragma clang fp contract(off)
    const double prod = du * dt;
    return u + prod;
}

template <class R, int V, bool TOP, int NS>
__global__ __launch_bounds__(256) void k_adjust_cf(AdjustArgs a)
{
#pragma clang fp contract(off)
    const size_t n = (size_t)a.ncol, ld = (size_t)a.ld, c = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (c >= n) return;
    const int nlay = a.nlay, k0 = (int)blockIdx.y * a.chunk, k1 = min(nlay, k0 + a.chunk);
    double dt[V], pb[V], nb[NS][V];         // dtsfc; pressure and net fluxes of the level below
    adjust_load<R, V>(a.dtsfc, c, dt);
#pragma unroll 2
    for (int k = k0; k <= k1; k++) {
        const size_t at = (size_t)(TOP ? nlay - k : k) * ld + c;
        const bool mine = k < k1 || k1 == nlay;          // (the chunk's last level is the next chunk's first)
        double p[V], net[NS][V];
        adjust_load<R, V>(a.plev, at, p);
#pragma unroll
        for (int s = 0; s < NS; s++) {
            double u[V], d[V], du[V];
            adjust_load<R, V>(a.s[s].u, at, u);
            adjust_load<R, V>(a.s[s].d, at, d);
            adjust_load<R, V>(a.s[s].du, at, du);
#pragma unroll
            for (int j = 0; j < V; j++) { u[j] = adjust_up(u[j], du[j], dt[j]); net[s][j] = u[j] - d[j]; }
            if (mine) adjust_store<R, V>(a.s[s].ua, at, u);
        }
        if (k > k0) {
            const size_t ah = (size_t)(TOP ? nlay - k : k - 1) * ld + c;         // layer k - 1
#pragma unroll
            for (int s = 0; s < NS; s++) {
                double h[V];
#pragma unroll
                for (int j = 0; j < V; j++) h[j] = a.heatfac * (nb[s][j] - net[s][j]) / (pb[j] - p[j]);
                adjust_store<R, V>(a.s[s].hr, ah, h);
            }
        }
#pragma unroll
        for (int j = 0; j < V; j++) {
            pb[j] = p[j];
#pragma unroll
            for (int s = 0; s < NS; s++) nb[s][j] = net[s][j];
        }
    }
}

template <class R, bool TOP, int NS>
__global__ __launch_bounds__(256) void k_adjust_lf(AdjustArgs a)
{
#pragma clang fp contract(off)
    constexpr int V = 16 / (int)sizeof(R);
    const size_t nlev = (size_t)a.nlay + 1, N = (size_t)a.ncol * nlev;
    const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (e0 >= N) return;
    const int nv = (int)min((size_t)V, N - e0);          // values of this thread (the run's last thread: fewer)
    // column and vertical index of the first value
    size_t i0;
    if (N <= 0xffffffffull) i0 = (unsigned)e0 / (unsigned)nlev; else i0 = e0 / nlev;
    const int kk0 = (int)(e0 - i0 * nlev);
    // slots 1 .. V: the thread's values; slot 0 (TOP) or V + 1: the neighbour that holds the level above the last of them
    double p[V + 2], net[NS][V + 2], dt[V + 2];
    size_t col[V + 2];
    int kk[V + 2];
    bool on[V + 2];
    {
        size_t i = i0; int q = kk0;
#pragma unroll
        for (int j = 1; j <= V; j++) { col[j] = i; kk[j] = q; on[j] = j <= nv; if (++q == (int)nlev) { q = 0; i++; } }
        // the neighbour counts only inside the same column; otherwise its slot is never used
        if constexpr (TOP) { on[0] = kk0 > 0; col[0] = i0; kk[0] = kk0 - 1; on[V + 1] = false; col[V + 1] = 0; kk[V + 1] = 0; }
        else { on[V + 1] = nv == V && kk[V] < (int)nlev - 1; col[V + 1] = col[V]; kk[V + 1] = kk[V] + 1; on[0] = false; col[0] = 0; kk[0] = 0; }
    }
    const bool wide = a.vec != 0 && nv == V;
    constexpr int X = TOP ? 0 : V + 1;                   // the neighbour's slot
#pragma unroll
    for (int j = 0; j < V + 2; j++) dt[j] = on[j] ? (double)static_cast<const R *>(a.dtsfc)[col[j]] : 0.0;
    auto load = [&](const void *src, double (&x)[V + 2]) {
        if (wide) {
            double v[V];
            adjust_load<R, V>(src, e0, v);
#pragma unroll
            for (int j = 0; j < V; j++) x[j + 1] = v[j];
        } else {
#pragma unroll
            for (int j = 1; j <= V; j++) x[j] = on[j] ? (double)static_cast<const R *>(src)[e0 + (size_t)(j - 1)] : 0.0;
        }
        x[TOP ? V + 1 : 0] = 0.0;
        x[X] = on[X] ? (double)static_cast<const R *>(src)[TOP ? e0 - 1 : e0 + (size_t)V] : 0.0;
    };
    load(a.plev, p);
#pragma unroll
    for (int s = 0; s < NS; s++) {
        double u[V + 2], d[V + 2], du[V + 2];
        load(a.s[s].u, u);
        load(a.s[s].d, d);
        load(a.s[s].du, du);
#pragma unroll
        for (int j = 0; j < V + 2; j++) { u[j] = adjust_up(u[j], du[j], dt[j]); net[s][j] = u[j] - d[j]; }
        if (wide) {
            double v[V];
#pragma unroll
            for (int j = 0; j < V; j++) v[j] = u[j + 1];
            adjust_store<R, V>(a.s[s].ua, e0, v);
        } else {
#pragma unroll
            for (int j = 1; j <= V; j++) if (on[j]) static_cast<R *>(a.s[s].ua)[e0 + (size_t)(j - 1)] = (R)u[j];
        }
    }
    // the layer above each of the thread's levels: between slot j (below) and slot j + 1, or j - 1 with TOP (above)
#pragma unroll
    for (int j = 1; j <= V; j++) {
        constexpr int UP = TOP ? -1 : 1;
        const bool has = on[j] && (TOP ? kk[j] > 0 : kk[j] < (int)nlev - 1);      // (the top level carries no layer; then slot j + UP is on)
        if (has) {
            const size_t ah = col[j] * (size_t)a.nlay + (size_t)(TOP ? kk[j] - 1 : kk[j]);
#pragma unroll
            for (int s = 0; s < NS; s++)
                static_cast<R *>(a.s[s].hr)[ah] = (R)(a.heatfac * (net[s][j] - net[s][j + UP]) / (p[j] - p[j + UP]));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_fill_rows : the host-pointer entries do not copy a row of an input array whose values are all the same for the columns of a batch
//               (well-mixed gases, cloud and aerosol arrays outside the cloudy / dusty layers): entry blockIdx.y of the table (pinned host
//               memory, written by the entry's host threads) names a run of such rows and the 8-byte pattern they hold.
// ------------------------------------------------------------------------------------------------
struct RowFill { unsigned long long *dst; unsigned long long n, bits; };
constexpr int FILL_BLOCKS = 64;
constexpr unsigned long long FILL_MAX = 1ull << 20;      // values per table entry (a longer run is several entries)
__global__ __launch_bounds__(256) void k_fill_rows(const RowFill *__restrict__ tab)
{
    const RowFill e = tab[blockIdx.y];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < e.n; i += (unsigned long long)FILL_BLOCKS * 256) e.dst[i] = e.bits;
}

// ------------------------------------------------------------------------------------------------
// k_widen_rows / k_narrow_rows : the *_r4 host-pointer entries (float32 host arrays).  A float32 row crosses PCIe as float32 into the
//               staging set's landing area and is widened into the float64 row the solver reads; a staged float64 output row is rounded
//               to nearest into the landing area and leaves as float32.  Entry blockIdx.y of the table (pinned host memory, like
//               k_fill_rows') names one row: its float64 address d, its float32 address f and its n values; gridDim.x workgroups share it.
//               A lane moves 16 bytes on the float32 side - four values - once the head has brought f to a 16-byte boundary (landing rows
//               start on one: no head there), and the 32 bytes on the float64 side as two 16-byte accesses where d is on such a boundary
//               too, as 8 + 16 + 8 where it is not (row r of a staged array starts at inner * nb * r doubles: on an 8-byte boundary only,
//               every other row, when inner * nb is odd).  Head and tail - at most three values each - go value by value.
// ------------------------------------------------------------------------------------------------
struct RowCvt { double *d; float *f; unsigned long long n; };
constexpr int CVT_BLOCKS = 64;                            // workgroups per table entry at most (the launch takes fewer for short rows)
constexpr unsigned long long CVT_LANE = 16;               // values a lane is meant to move: what the launch sizes gridDim.x by
__device__ __forceinline__ unsigned long long cvt_head(const float *f, unsigned long long n)
{
    const unsigned long long h = ((16u - (unsigned)(reinterpret_cast<uintptr_t>(f) & 15u)) & 15u) >> 2;
    return h < n ? h : n;
}
__global__ __launch_bounds__(256) void k_widen_rows(const RowCvt *__restrict__ tab)
{
    const RowCvt e = tab[blockIdx.y];
    const unsigned long long head = cvt_head(e.f, e.n), nv = (e.n - head) / 4;
    const float *f = e.f + head;
    double *d = e.d + head;
    const bool d16 = (reinterpret_cast<uintptr_t>(d) & 15u) == 0;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (unsigned long long)gridDim.x * 256) {
        const float4 x = *reinterpret_cast<const float4 *>(f + 4 * v);
        double *o = d + 4 * v;
        if (d16) {
            *reinterpret_cast<double2 *>(o) = make_double2((double)x.x, (double)x.y);
            *reinterpret_cast<double2 *>(o + 2) = make_double2((double)x.z, (double)x.w);
        } else {
            o[0] = (double)x.x;
            *reinterpret_cast<double2 *>(o + 1) = make_double2((double)x.y, (double)x.z);
            o[3] = (double)x.w;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        const unsigned long long t = threadIdx.x, t1 = head + 4 * nv + t;
        if (t < head) e.d[t] = (double)e.f[t];
        if (t1 < e.n) e.d[t1] = (double)e.f[t1];
    }
}
__global__ __launch_bounds__(256) void k_narrow_rows(const RowCvt *__restrict__ tab)
{
    const RowCvt e = tab[blockIdx.y];
    const unsigned long long head = cvt_head(e.f, e.n), nv = (e.n - head) / 4;
    float *f = e.f + head;
    const double *d = e.d + head;
    const bool d16 = (reinterpret_cast<uintptr_t>(d) & 15u) == 0;
    for (unsigned long long v = (unsigned long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (unsigned long long)gridDim.x * 256) {
        const double *i = d + 4 * v;
        float4 x;
        if (d16) {
            const double2 a = *reinterpret_cast<const double2 *>(i), b = *reinterpret_cast<const double2 *>(i + 2);
            x = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
        } else {
            const double a = i[0];
            const double2 b = *reinterpret_cast<const double2 *>(i + 1);
            const double c = i[3];
            x = make_float4((float)a, (float)b.x, (float)b.y, (float)c);
        }
        *reinterpret_cast<float4 *>(f + 4 * v) = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        const unsigned long long t = threadIdx.x, t1 = head + 4 * nv + t;
        if (t < head) e.f[t] = (float)e.d[t];
        if (t1 < e.n) e.f[t1] = (float)e.d[t1];
    }
}

// ------------------------------------------------------------------------------------------------
// k_form_in / k_form_out : the *_as entries (include/rrtmg_lw_hip.h, rrtmg_lw_hip_array_form).  One launch brings every input array of
//               a column batch from the caller's form (float32 or float64; reference order or column-slowest C order; surface or top
//               first) into the float64 reference form, nb columns wide, that the solver's kernels read; one launch takes the staged
//               outputs back.  The table - one entry per array, passed by value - names the arrays; a workgroup finds its array from its
//               block index and moves one tile of it.
//   FA_PLANE    reference form (column, row) at column + nb * row, row = k + V * b (k: vertical index of V, b: trailing index of
//               `inner`: 16 bands, NG g-points).  Reference-order caller: the same rows, ncol wide.  Column-slowest caller: the column's
//               V * inner values lie together, at kk * inner + b - a transposition of 64 columns x 64 values through LDS, so that the
//               loads run along the caller's fastest index and the stores along the columns.  The tile's rows are padded by one value
//               (65 doubles = 130 dwords: the 32 lanes of a ds_read_b64 group that walk down a tile column fall on 32 different bank pairs).
//   FA_TAUCLD   taucld, whose 16 bands are fastest in both forms ((16, ncol, nlay) | (ncol, nlay, 16)): they move as units, no LDS.
//   FA_TAUCTOT  taucld again, where the solver reads only its band sum (inflglw >= 1, GcmIn::tauctot): the sum is formed here in the
//               reference's order (src/rrtmg_lw_cldprop.f90:173-186) and one value per cell is staged.
//   With `flip` the caller's vertical index runs from the top: reference k lies at V - 1 - k.  Offsets into the caller's arrays are
//   64-bit (1e6 x 137 x 16 elements); threads past the batch's last column or the array's last row neither load nor store.
// ------------------------------------------------------------------------------------------------
enum { FA_PLANE = 0, FA_TAUCLD = 1, FA_TAUCTOT = 2 };
struct FormArray {
    void *user;                 // the caller's array (all ncol columns)
    double *staged;             // the batch's columns in reference form
    int V, inner, kind, flip;
    unsigned tile0;             // first workgroup of this array
};
constexpr int FORM_MAX = 26;
constexpr int FORM_TILE = 64;
struct FormTable {
    FormArray a[FORM_MAX];
    int n;                      // arrays
    int nb;                     // columns of the batch (width of the staged arrays)
    int layer_fastest;
    unsigned long long ncol, col0;      // the caller's columns, the batch's first
};
template <class T> __device__ __forceinline__ double form_load(const void *p, unsigned long long i) { return (double)((const T *)p)[i]; }
template <class T> __device__ __forceinline__ void form_store(void *p, unsigned long long i, double v) { ((T *)p)[i] = (T)v; }
// the caller's row (reference order) or offset inside the column (column-slowest order) of reference row r = k + V * b, and back
__device__ __forceinline__ unsigned form_user_of(const FormArray &e, unsigned r, bool lf)
{
    const unsigned b = r / (unsigned)e.V, k = r - b * (unsigned)e.V, kk = e.flip ? (unsigned)e.V - 1u - k : k;
    return lf ? kk * (unsigned)e.inner + b : kk + (unsigned)e.V * b;
}
__device__ __forceinline__ unsigned form_row_of(const FormArray &e, unsigned j)      // column-slowest offset j = kk * inner + b -> r
{
    const unsigned kk = j / (unsigned)e.inner, b = j - kk * (unsigned)e.inner, k = e.flip ? (unsigned)e.V - 1u - kk : kk;
    return k + (unsigned)e.V * b;
}
__device__ __forceinline__ int form_find(const FormTable &t)
{
    int a = 0;
    while (a + 1 < t.n && blockIdx.x >= t.a[a + 1].tile0) a++;
    return a;
}

template <class T>
__global__ __launch_bounds__(256) void k_form_in(const FormTable t)
{
    __shared__ double tile[FORM_TILE][FORM_TILE + 1];
    const FormArray e = t.a[form_find(t)];
    const bool lf = t.layer_fastest != 0;
    const unsigned nb = (unsigned)t.nb, nct = (nb + FORM_TILE - 1) / FORM_TILE;
    const unsigned tl = blockIdx.x - e.tile0, ct = tl % nct, jt = tl / nct;
    const unsigned lane = threadIdx.x & 63u, ty = threadIdx.x >> 6;
    const unsigned long long ncol = t.ncol, col0 = t.col0;
    if (e.kind == FA_TAUCLD) {           // jt: the reference layer; 64 columns x 16 bands
        const unsigned k = jt, kk = e.flip ? (unsigned)e.V - 1u - k : k;
#pragma unroll
        for (unsigned it = 0; it < 4; it++) {
            const unsigned el = threadIdx.x + 256u * it, col = ct * FORM_TILE + (el >> 4), b = el & 15u;
            if (col >= nb) continue;
            const unsigned long long cell = lf ? (col0 + col) * (unsigned long long)e.V + kk : (col0 + col) + ncol * kk;
            e.staged[(size_t)NBND * ((size_t)col + (size_t)nb * k) + b] = form_load<T>(e.user, cell * NBND + b);
        }
        return;
    }
    const unsigned R = e.kind == FA_TAUCTOT ? (unsigned)e.V : (unsigned)e.V * (unsigned)e.inner;      // staged rows
    if (!lf) {                           // the caller's rows are the reference's: lanes along the columns on both sides
        const unsigned col = ct * FORM_TILE + lane;
#pragma unroll 4
        for (unsigned it = 0; it < FORM_TILE / 4; it++) {
            const unsigned r = jt * FORM_TILE + ty + 4u * it;
            if (col >= nb || r >= R) continue;
            double v;
            if (e.kind == FA_TAUCTOT) {
                const unsigned kk = e.flip ? (unsigned)e.V - 1u - r : r;
                const unsigned long long p = ((col0 + col) + ncol * kk) * NBND;
                double sum = 0.0;
                for (int ib = 0; ib < NBND; ib++) sum = sum + form_load<T>(e.user, p + ib);
                v = sum;
            } else v = form_load<T>(e.user, (col0 + col) + ncol * form_user_of(e, r, false));
            e.staged[(size_t)col + (size_t)nb * r] = v;
        }
        return;
    }
    // column-slowest caller: loads along the column's own values, stores along the columns
#pragma unroll 4
    for (unsigned it = 0; it < FORM_TILE / 4; it++) {
        const unsigned c = ty + 4u * it, col = ct * FORM_TILE + c, j = jt * FORM_TILE + lane;
        if (col >= nb || j >= R) continue;
        double v;
        if (e.kind == FA_TAUCTOT) {
            const unsigned long long p = ((col0 + col) * (unsigned long long)e.V + j) * NBND;
            double sum = 0.0;
            for (int ib = 0; ib < NBND; ib++) sum = sum + form_load<T>(e.user, p + ib);
            v = sum;
        } else v = form_load<T>(e.user, (col0 + col) * (unsigned long long)R + j);
        tile[c][lane] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (unsigned it = 0; it < FORM_TILE / 4; it++) {
        const unsigned jj = ty + 4u * it, col = ct * FORM_TILE + lane, j = jt * FORM_TILE + jj;
        if (col >= nb || j >= R) continue;
        const unsigned r = e.kind == FA_TAUCTOT ? (e.flip ? (unsigned)e.V - 1u - j : j) : form_row_of(e, j);
        e.staged[(size_t)col + (size_t)nb * r] = tile[lane][jj];
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_form_out(const FormTable t)          // FA_PLANE arrays only
{
    __shared__ double tile[FORM_TILE][FORM_TILE + 1];
    const FormArray e = t.a[form_find(t)];
    const bool lf = t.layer_fastest != 0;
    const unsigned nb = (unsigned)t.nb, nct = (nb + FORM_TILE - 1) / FORM_TILE;
    const unsigned tl = blockIdx.x - e.tile0, ct = tl % nct, jt = tl / nct;
    const unsigned lane = threadIdx.x & 63u, ty = threadIdx.x >> 6;
    const unsigned long long ncol = t.ncol, col0 = t.col0;
    const unsigned R = (unsigned)e.V * (unsigned)e.inner;
    if (!lf) {
        const unsigned col = ct * FORM_TILE + lane;
#pragma unroll 4
        for (unsigned it = 0; it < FORM_TILE / 4; it++) {
            const unsigned r = jt * FORM_TILE + ty + 4u * it;
            if (col >= nb || r >= R) continue;
            form_store<T>(e.user, (col0 + col) + ncol * form_user_of(e, r, false), e.staged[(size_t)col + (size_t)nb * r]);
        }
        return;
    }
#pragma unroll 4
    for (unsigned it = 0; it < FORM_TILE / 4; it++) {          // loads along the columns (a tile row per value of the column) ...
        const unsigned jj = ty + 4u * it, col = ct * FORM_TILE + lane, j = jt * FORM_TILE + jj;
        if (col >= nb || j >= R) continue;
        tile[jj][lane] = e.staged[(size_t)col + (size_t)nb * form_row_of(e, j)];
    }
    __syncthreads();
#pragma unroll 4
    for (unsigned it = 0; it < FORM_TILE / 4; it++) {          // ... stores along the column's own values
        const unsigned c = ty + 4u * it, col = ct * FORM_TILE + c, j = jt * FORM_TILE + lane;
        if (col >= nb || j >= R) continue;
        form_store<T>(e.user, (col0 + col) * (unsigned long long)R + j, tile[lane][c]);
    }
}

// ------------------------------------------------------------------------------------------------
// k_solve / k_solve_flux : rrtmg_lw_hip_solve* - fluxes and heating rates from the CALLER's optical depths and sources: the level loops
//               of rtrn (cloud = 1, src/rrtmg_lw_rtrn.f90:361-540) and rtrnmc (cloud = 2, src/rrtmg_lw_rtrnmc.f90) in float64 on the float64
//               tables (T.sl.lut {exp_tbl, tfn_tbl}, T.sl.tau_tbl), every operation rounding on its own (contract(off)).  Kernels of their
//               own: no cell codes, nothing shared with k_sweepc / k_sweepz / k_layer.
//   k_solve       one thread per (column, band), lanes = consecutive columns (every load a coalesced row), blockIdx.y = band.  A thread
//               takes its band's g-points four at a time (SOLVE_CHUNK: their radiances stay in registers; all sixteen at once spilt)
//               down and up through the levels and adds each level's sum over the chunk to the band's partial, which it alone
//               touches.  Nothing indexed by level is kept: the upward sweep reads tau and fracs again and forms atrans, atot and the
//               source terms again - the same numbers - (2 x 16 B per cell and sweep) rather than writing and reading four values
//               per cell (64 B).  A column's lanes exchange nothing.
//   k_solve_flux  one thread per column: the band sum (x wtdiff x delwave, then x fluxfac - rtrn :549-604), net fluxes, heating rates.
//   Element offsets are 64-bit throughout (size_t): ncol x nlay x NG passes 2^31.  Threads past the batch's last column return first.
// ------------------------------------------------------------------------------------------------
struct SolveArgs {
    const double *plev, *emis, *tau, *fracs, *planklay, *planklev, *plankbnd, *dplankbnd_dt, *cldfr, *odcld;    // the caller's, at the batch's first column
    const unsigned *submask;
    double *uflx, *dflx, *hr, *uflxc, *dflxc, *hrc, *duflx_dt, *duflxc_dt;                                      // (k_solve_flux)
    double *part;                       // [SV_N][16][nlay + 1][nb]  sums over a band's g-points; the slots a call does not form are not there
    unsigned long long nb, ld;          // columns of the batch, column extent of the caller's arrays
    int nlay, cloud;
    int slot[6];                        // where u, d, uc, dc, du, duc lie in `part` (clear = total where the streams coincide), -1: not formed
};
enum { SV_U, SV_D, SV_UC, SV_DC, SV_DU, SV_DUC };

// what rtrn forms of one cell: the gas and total absorptivities and the Planck source terms towards both interfaces
struct SolveCell { double atrans, atot, bbd, bbdtot, bbugas, bbutot, gassrc; };

// table position of an optical depth: lut_index, kept inside the table whatever the value (a non-finite one poisons the cell instead)
__device__ __forceinline__ int solve_index(double od, double bpade)
{
    const int i = lut_index(od, bpade);
    return i < 0 ? 0 : i > 10000 ? 10000 : i;
}

__device__ __forceinline__ SolveCell solve_cell(const double *__restrict__ lut, const double *__restrict__ tau_tbl, double bpade, bool cldy,
                                                double odepth, double odc, double plfrac, double blay, double dplankup, double dplankdn)
{
#pragma clang fp contract(off)
    const double rec_6 = 0.166667;
    SolveCell c;
    const double poison = (odepth - odepth) + (odc - odc);      // 0, or NaN where an optical depth is infinite or NaN: it has no table position
    if (odepth < 0.0) odepth = 0.0;
    if (cldy) {
        double odtot = odepth + odc;
        if (odtot < 0.06) {
            c.atrans = odepth - 0.5 * odepth * odepth;
            const double odepth_rec = rec_6 * odepth;
            c.bbd = plfrac * (blay + dplankdn * odepth_rec);
            c.gassrc = c.bbd * c.atrans;
            c.atot = odtot - 0.5 * odtot * odtot;
            const double odtot_rec = rec_6 * odtot;
            c.bbdtot = plfrac * (blay + dplankdn * odtot_rec);
            c.bbugas = plfrac * (blay + dplankup * odepth_rec);
            c.bbutot = plfrac * (blay + dplankup * odtot_rec);
        } else if (odepth <= 0.06) {
            c.atrans = odepth - 0.5 * odepth * odepth;
            const double odepth_rec = rec_6 * odepth;
            c.bbd = plfrac * (blay + dplankdn * odepth_rec);
            c.gassrc = c.bbd * c.atrans;
            const int ittot = solve_index(odtot, bpade);
            const double tfactot = lut[2 * ittot + 1];
            c.bbdtot = plfrac * (blay + tfactot * dplankdn);
            c.atot = 1. - lut[2 * ittot];
            c.bbugas = plfrac * (blay + dplankup * odepth_rec);
            c.bbutot = plfrac * (blay + tfactot * dplankup);
        } else {
            const int itgas = solve_index(odepth, bpade);
            odepth = tau_tbl[itgas];
            c.atrans = 1. - lut[2 * itgas];
            const double tfacgas = lut[2 * itgas + 1];
            c.gassrc = c.atrans * plfrac * (blay + tfacgas * dplankdn);
            odtot = odepth + odc;
            const int ittot = solve_index(odtot, bpade);
            const double tfactot = lut[2 * ittot + 1];
            c.bbdtot = plfrac * (blay + tfactot * dplankdn);
            c.bbd = plfrac * (blay + tfacgas * dplankdn);
            c.atot = 1. - lut[2 * ittot];
            c.bbugas = plfrac * (blay + tfacgas * dplankup);
            c.bbutot = plfrac * (blay + tfactot * dplankup);
        }
    } else {
        c.atot = 0.0; c.bbdtot = 0.0; c.bbutot = 0.0; c.gassrc = 0.0;
        if (odepth <= 0.06) {
            c.atrans = odepth - 0.5 * odepth * odepth;
            odepth = rec_6 * odepth;
            c.bbd = plfrac * (blay + dplankdn * odepth);
            c.bbugas = plfrac * (blay + dplankup * odepth);
        } else {
            const int itr = solve_index(odepth, bpade);
            c.atrans = 1. - lut[2 * itr];
            const double tausfac = lut[2 * itr + 1];
            c.bbd = plfrac * (blay + tausfac * dplankdn);
            c.bbugas = plfrac * (blay + tausfac * dplankup);
        }
    }
    if (poison != 0.0) c.atrans = poison;
    return c;
}

// the cloud terms of a level: rtrn's per layer, rtrnmc's per g-point from the sub-column mask (solve_bit)
struct SolveCloud { bool cldy; double cf, odc, efc; };
__device__ __forceinline__ SolveCloud solve_cloud(const SolveArgs &a, size_t i, int k, int b)
{
#pragma clang fp contract(off)
    SolveCloud c{};
    if (a.cloud == 0) return c;
    const size_t ld = (size_t)a.ld, L = (size_t)a.nlay;
    if (a.cloud == 1) {
        c.cf = a.cldfr[i + ld * (size_t)k];
        c.cldy = c.cf >= 1.e-6;
    } else {
        unsigned any = 0;
#pragma unroll
        for (int w = 0; w < MASK_WORDS; w++) {
            unsigned m = a.submask[i + ld * ((size_t)k + L * (size_t)w)];
            if (w == MASK_WORDS - 1 && (NGPT & 31) != 0) m &= (1u << (NGPT & 31)) - 1u;
            any |= m;
        }
        c.cldy = any != 0;
        c.cf = 1.0;
    }
    if (c.cldy) {
        c.odc = a.odcld[i + ld * ((size_t)k + L * (size_t)b)];
        c.efc = (1. - exp(-c.odc)) * c.cf;
    }
    return c;
}
// bit g of the mask of (column i, layer k): g < NGPT
__device__ __forceinline__ bool solve_bit(const SolveArgs &a, size_t i, int k, int g)
{
    return ((a.submask[i + (size_t)a.ld * ((size_t)k + (size_t)a.nlay * (size_t)(g >> 5))] >> (g & 31)) & 1u) != 0;
}

constexpr int SOLVE_CHUNK = 4;          // g-points a thread carries through the levels at a time

template <int IDRV>
__global__ __launch_bounds__(64) void k_solve(const DevTables T, const SolveArgs a)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (size_t)a.nb) return;
    const int b = blockIdx.y, nlay = a.nlay;
    const int ng = T.band[b].ng, g0 = T.band[b].gstart;
    const size_t ld = (size_t)a.ld, L = (size_t)nlay, nb = (size_t)a.nb, nlev = L + 1;
    const double *__restrict__ lut = T.stat + T.sl.lut;
    const double *__restrict__ tau_tbl = T.stat + T.sl.tau_tbl;
    const double bpade = T.bpade;
    const bool mc = a.cloud == 2;
    const bool clr = a.slot[SV_DC] >= 0 && a.slot[SV_DC] != a.slot[SV_D];      // a clear-sky stream of its own
    constexpr int CH = SOLVE_CHUNK, ND = IDRV ? CH : 1;
    const double plankbnd = a.plankbnd[i + ld * (size_t)b], reflect = 1. - a.emis[i + ld * (size_t)b];
    const double dplankbnd = IDRV ? a.dplankbnd_dt[i + ld * (size_t)b] : 0.0;

    // The band's g-points CH at a time, each chunk down and up through all levels; a level's sum over the chunk is added to the band's
    // partial, which only this thread touches (the first chunk stores): the order of the sum is fixed, a column's lanes exchange nothing.
    for (int j0 = 0; j0 < ng; j0 += CH) {
        const bool first = j0 == 0;
        const auto put = [&](int v, size_t lev, double x) {
            double *p = a.part + (((size_t)a.slot[v] * NBND + (size_t)b) * nlev + lev) * nb + i;
            *p = first ? x : *p + x;
        };
        double radld[CH], radclrd[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) { radld[j] = 0.0; radclrd[j] = 0.0; }
        bool iclddn = false;
        if (first) { put(SV_D, L, 0.0); if (clr) put(SV_DC, L, 0.0); }
        for (int lev = nlay; lev >= 1; lev--) {                     // rtrn :361-466
            const int k = lev - 1;
            const double blay = a.planklay[i + ld * ((size_t)k + L * (size_t)b)];
            const double dplankup = a.planklev[i + ld * ((size_t)lev + nlev * (size_t)b)] - blay;
            const double dplankdn = a.planklev[i + ld * ((size_t)k + nlev * (size_t)b)] - blay;
            const SolveCloud cl = solve_cloud(a, i, k, b);
            if (cl.cldy) iclddn = true;
            double sd = 0.0, sdc = 0.0;
#pragma unroll
            for (int j = 0; j < CH; j++) {
                if (j0 + j < ng) {
                    const int g = g0 + j0 + j;
                    const size_t at = i + ld * ((size_t)k + L * (size_t)g);
                    const bool bit = !mc || (cl.cldy && solve_bit(a, i, k, g));
                    const double cf = bit ? cl.cf : 0.0, odc = bit ? cl.odc : 0.0, efc = bit ? cl.efc : 0.0;
                    const SolveCell c = solve_cell(lut, tau_tbl, bpade, cl.cldy, a.tau[at], odc, a.fracs[at], blay, dplankup, dplankdn);
                    if (cl.cldy) radld[j] = radld[j] - radld[j] * (c.atrans + efc * (1. - c.atrans)) + c.gassrc + cf * (c.bbdtot * c.atot - c.gassrc);
                    else radld[j] = radld[j] + (c.bbd - radld[j]) * c.atrans;
                    sd = sd + radld[j];
                    if (iclddn) radclrd[j] = radclrd[j] + (c.bbd - radclrd[j]) * c.atrans;
                    else radclrd[j] = radld[j];
                    sdc = sdc + radclrd[j];
                }
            }
            put(SV_D, (size_t)k, sd);
            if (clr) put(SV_DC, (size_t)k, sdc);
        }
        // the surface, rtrn :476-495
        double radlu[CH], radclru[CH], dlu[ND], dclru[ND];
        {
            double su = 0.0, suc = 0.0, sdu = 0.0;
#pragma unroll
            for (int j = 0; j < CH; j++) {
                radlu[j] = 0.0; radclru[j] = 0.0;
                if (IDRV) { dlu[IDRV ? j : 0] = 0.0; dclru[IDRV ? j : 0] = 0.0; }
                if (j0 + j < ng) {
                    const double f1 = a.fracs[i + ld * (L * (size_t)(g0 + j0 + j))];
                    const double rad0 = f1 * plankbnd;
                    radlu[j] = rad0 + reflect * radld[j];
                    radclru[j] = rad0 + reflect * radclrd[j];
                    su = su + radlu[j];
                    suc = suc + radclru[j];
                    if (IDRV) { dlu[IDRV ? j : 0] = f1 * dplankbnd; dclru[IDRV ? j : 0] = dlu[IDRV ? j : 0]; sdu = sdu + dlu[IDRV ? j : 0]; }
                }
            }
            put(SV_U, 0, su);
            if (clr) put(SV_UC, 0, suc);
            if (IDRV) { put(SV_DU, 0, sdu); if (clr) put(SV_DUC, 0, sdu); }
        }
        for (int lev = 1; lev <= nlay; lev++) {                     // rtrn :497-540
            const int k = lev - 1;
            const double blay = a.planklay[i + ld * ((size_t)k + L * (size_t)b)];
            const double dplankup = a.planklev[i + ld * ((size_t)lev + nlev * (size_t)b)] - blay;
            const double dplankdn = a.planklev[i + ld * ((size_t)k + nlev * (size_t)b)] - blay;
            const SolveCloud cl = solve_cloud(a, i, k, b);
            double su = 0.0, suc = 0.0, sdu = 0.0, sduc = 0.0;
#pragma unroll
            for (int j = 0; j < CH; j++) {
                if (j0 + j < ng) {
                    const int g = g0 + j0 + j;
                    const size_t at = i + ld * ((size_t)k + L * (size_t)g);
                    const bool bit = !mc || (cl.cldy && solve_bit(a, i, k, g));
                    const double cf = bit ? cl.cf : 0.0, odc = bit ? cl.odc : 0.0, efc = bit ? cl.efc : 0.0;
                    const SolveCell c = solve_cell(lut, tau_tbl, bpade, cl.cldy, a.tau[at], odc, a.fracs[at], blay, dplankup, dplankdn);
                    if (cl.cldy) {
                        const double gassrc = c.bbugas * c.atrans;
                        radlu[j] = radlu[j] - radlu[j] * (c.atrans + efc * (1. - c.atrans)) + gassrc + cf * (c.bbutot * c.atot - gassrc);
                        if (IDRV) dlu[IDRV ? j : 0] = dlu[IDRV ? j : 0] * cf * (1.0 - c.atot) + dlu[IDRV ? j : 0] * (1.0 - cf) * (1.0 - c.atrans);
                    } else {
                        radlu[j] = radlu[j] + (c.bbugas - radlu[j]) * c.atrans;
                        if (IDRV) dlu[IDRV ? j : 0] = dlu[IDRV ? j : 0] * (1.0 - c.atrans);
                    }
                    su = su + radlu[j];
                    if (iclddn) radclru[j] = radclru[j] + (c.bbugas - radclru[j]) * c.atrans;
                    else radclru[j] = radlu[j];
                    suc = suc + radclru[j];
                    if (IDRV) {
                        sdu = sdu + dlu[IDRV ? j : 0];
                        if (iclddn) dclru[IDRV ? j : 0] = dclru[IDRV ? j : 0] * (1.0 - c.atrans);
                        else dclru[IDRV ? j : 0] = dlu[IDRV ? j : 0];
                        sduc = sduc + dclru[IDRV ? j : 0];
                    }
                }
            }
            put(SV_U, (size_t)lev, su);
            if (clr) put(SV_UC, (size_t)lev, suc);
            if (IDRV) { put(SV_DU, (size_t)lev, sdu); if (clr) put(SV_DUC, (size_t)lev, sduc); }
        }
    }
}

__global__ __launch_bounds__(64) void k_solve_flux(const DevTables T, const SolveArgs a)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (size_t)a.nb) return;
    const size_t ld = (size_t)a.ld, nb = (size_t)a.nb, nlev = (size_t)a.nlay + 1;
    const double wtdiff = 0.5;
    const bool clear = a.uflxc != nullptr, deriv = a.slot[SV_DU] >= 0;
    double netp = 0.0, netcp = 0.0, pp = 0.0;
    for (size_t lev = 0; lev < nlev; lev++) {
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 6; q++) {
            if (a.slot[q] < 0 || (!clear && (q == SV_UC || q == SV_DC))) continue;
            const double *p = a.part + ((size_t)a.slot[q] * NBND * nlev + lev) * nb + i;
            for (int b = 0; b < NBND; b++) {
                const double f = p[(size_t)b * nlev * nb] * wtdiff;
                if (q >= SV_DU) v[q] = v[q] + f * T.delwave[b] * T.fluxfac;      // rtrn :566-574
                else v[q] = v[q] + f * T.delwave[b];                             // rtrn :549-562
            }
            if (q < SV_DU) v[q] = v[q] * T.fluxfac;                              // rtrn :580-596
        }
        const size_t o = i + ld * lev;
        const double p = a.plev[o];
        a.uflx[o] = v[SV_U]; a.dflx[o] = v[SV_D];
        const double net = v[SV_U] - v[SV_D], netc = v[SV_UC] - v[SV_DC];
        if (clear) { a.uflxc[o] = v[SV_UC]; a.dflxc[o] = v[SV_DC]; }
        if (deriv) { a.duflx_dt[o] = v[SV_DU]; a.duflxc_dt[o] = v[SV_DUC]; }
        if (lev > 0) {                                                          // rtrn :597-604
            a.hr[o - ld] = T.heatfac * (netp - net) / (pp - p);
            if (clear) a.hrc[o - ld] = T.heatfac * (netcp - netc) / (pp - p);
        }
        netp = net; netcp = netc; pp = p;
    }
}

}  // namespace rrlw
