// C-ABI implementation (include/rrtmg_lw_hip.h): device state, workspace, batching, kernel dispatch.
// Replaces the serial `do iplon = 1, ncol` loop of the reference's rrtmg_lw
// (src/rrtmg_lw_rad.nomcica.f90:472-586) with batched launches of the kernels in kernels.hip.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <sched.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdint>
#include <cstdarg>
#include <mutex>
#include <string>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/rrtmg_lw_hip.h"
#include "kernels.hip"
#include "mtjump.hpp"
#include "hostrows.hpp"
#include "owned.hpp"

namespace {

using namespace rrlw;

constexpr int BLOCK = 256;
// columns per batch of the host-pointer entries (H2D | kernels | D2H pipeline); RRTMG_LW_HOST_BATCH overrides (measurements)
const int HOST_BATCH = []() { const char *e = getenv("RRTMG_LW_HOST_BATCH"); const int v = e ? atoi(e) : 0; return v >= 64 ? v : 16384; }();     // 16 384: the entries are bound by the host threads, short batches fill and drain the pipeline sooner (524 288 columns pinned: 93.8 ms against 119.6 with 32 768)

// staging sets of the host-pointer pipeline (device staging, pinned host staging, events): the calling thread may be this many batches
// ahead of the batch whose outputs it unpacks.  With two, the thread's waits at the head of every iteration (the H2D of batch i - 2 out of
// the pinned set, the D2H of batch i - 2 into it) left the copy engines and the kernels taking turns: a trace of a 524 288-column call
// showed 11 ms of overlap between 44 ms of kernels and 52 ms of copies.
constexpr int HOST_SETS = 4;

// ---- who owns what ------------------------------------------------------------------------------------------------------------------
// Every GPU resource of the driver is held by an owner (owned.hpp) over one of these traits; the release calls appear here and nowhere
// else in this file.  release / acquire hand the hipError_t back as an int: a growth site reports it through fail() (grow, drop), a
// destructor or a move-assignment - finalize_state, a re-initialisation - ignores it.
struct DevMemTraits {       // (an earlier launch may still use the buffer: the device is idle before it goes)
    using handle = void *;
    static int acquire(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static int release(void *p) { const hipError_t s = hipDeviceSynchronize(), f = hipFree(p); return (int)(s != hipSuccess ? s : f); }
};
struct PinnedTraits {
    using handle = void *;
    static int acquire(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static int release(void *p) { return (int)hipHostFree(p); }
};
struct StreamTraits { using handle = hipStream_t; static int release(hipStream_t s) { return (int)hipStreamDestroy(s); } };
struct EventTraits { using handle = hipEvent_t; static int release(hipEvent_t e) { return (int)hipEventDestroy(e); } };
struct GraphTraits { using handle = hipGraph_t; static int release(hipGraph_t g) { return (int)hipGraphDestroy(g); } };
struct GraphExecTraits { using handle = hipGraphExec_t; static int release(hipGraphExec_t g) { return (int)hipGraphExecDestroy(g); } };
using DevBuf = owned::GrowBuf<DevMemTraits>;
using PinnedBuf = owned::GrowBuf<PinnedTraits>;
using Stream = owned::Owned<StreamTraits>;
using Event = owned::Owned<EventTraits>;
using Graph = owned::Owned<GraphTraits>;
using GraphExec = owned::Owned<GraphExecTraits>;

// the kissvec generator's jump tables on a device: one slot per (draws per sub-column, permuteseed) pair, the slots in one allocation made
// at the first use.  More slots than a call can have samples (RRTMG_LW_HIP_MAX_SAMPLES), so that the seeds of an averaging call and the
// single seed of a call made between two of them all stay.
constexpr int KISS_SLOTS = 2 * RRTMG_LW_HIP_MAX_SAMPLES;
struct KissSlot { unsigned long long stride = 0; long long seed = -1; unsigned long long used = 0; };
struct KissTable { std::vector<KissSlot> slot; unsigned long long clock = 0; DevBuf dev; PinnedBuf host; };      // host: the tables as built, page-locked (they are copied asynchronously)

// Columns per internal batch when the caller has not chosen (rrtmg_lw_hip_set_batch(0) comes back to this): 262 144 at up to 96 layers,
// the next lower power of two of 262 144 x 72 / nlay above (131 072 at 137 layers) - the workspace grows with the layers, the step
// time does not need it.  Measured (profiles/round5_batch_sweep.md, 1e6 columns, 32 768 / 65 536 / 131 072 / 262 144 per batch): cloudy
// 66.1 / 61.3 / 59.3 / 58.9 ms, clear 46.4 / 43.6 / 42.1 / 39.7, deep clouds 83.5 / 77.8 / 76.0 / 74.4; 137 layers with aerosol and
// d/dT (5e5 columns) 68.5 / 65.9 / 65.0 / 65.2.
constexpr int DEFAULT_BATCH = 262144;
struct State {
    bool init = false;
    int device = -1;
    HostTables H;
    DevTables D;
    DevBuf d_ktab, d_stat;
    // workspace: the allocation, the view of it the kernels receive, and the call shapes it was built for (ensure_workspace) - value-reset
    // wherever the allocation goes
    Workspace W{};
    DevBuf ws_buf;
    struct WsShape {
        int nlay = 0, ncolb = 0;
        bool cloud = false, mc = false, gdp = false, efcl = false, ovl = false;
        bool two_scr = false;        // it holds the second scratch set that split_sweep needs
        int groups = 0;
        size_t slabcols = 0;         // capacity of each partial slab array (gdn1 ..) in columns x slabs: `groups` wide slabs, or - a small batch whose
                                     // bands leave a slab each (split sweeps) - sixteen narrow ones
    } ws;
    // the gas-optics entries' own small workspace (k_colprep's per-column terms, k_optics' wide-window list): none of the solver's
    // codes, partials or cloud arrays
    DevBuf opt_buf;
    int opt_nlay = 0, opt_ncolb = 0;
    double *opt_percol = nullptr;
    int *opt_laytrop = nullptr, *opt_wide = nullptr;
    DevBuf d_err;
    // per-column / cloud-property arrays exist twice: k_colprep + k_cloudscan / k_cloudlay of batch i+1 run on `aux` while batch i is in k_layer/k_sweep
    struct PrepSet { double *percol; int *laytrop, *ncbands; double *odcld, *efcl; int *cflag; int *btop, *order, *hgrp, *hblk, *bbot, *hbot; double2 *ovl; int *perm, *wsort; double *tlayc, *tlevc, *cldfc; int *wide; } prep[2] = {};
    // the per-cell scratch written by k_layer and read by the sweeps exists twice as well: sweeps / k_flux of batch i (HBM-bound)
    // run on `sw` while k_layer of batch i+1 (latency-bound) runs on the caller's stream
    struct ScrSet { unsigned *scr[NSCR]; unsigned *fw; } scrset[2] = {};
    Stream aux;
    // streams of the sweep launches: `main` (the split pipeline's sweep stream) and q[0..2], on which the launches of the 3-, 2- and 1-quad
    // bands run beside the 4-quad launch.  Set 0 may use the whole chip; set 1 exists with a CU partition (rrtmg_lw_hip_set_cu_partition)
    // and is confined to the sweeps' share of the CUs.
    struct SweepSet { Stream main, q[3]; Event go, done[3]; } swset[2];
    // k_layer's streams of the partitioned pipeline: lay_u the whole chip (first batch of a call: nothing runs beside it), lay_m its share
    Stream lay_u, lay_m;
    int cu_layer = 0;            // CUs of k_layer's share (0: no partition), set by rrtmg_lw_hip_set_cu_partition
    int cu_total = 0;
    bool sweep_fanout = true;
    Event ev_last;                          // end of the previous device-entry call (calls on different streams share the workspace)
    Event ev_fork, ev_join;                               // run_prep: k_colprep beside k_cloudscan in a single-batch call
    bool ev_last_valid = false;
    Event ev_in, ev_ready[2], ev_layer[2], ev_done[2];
    // McICA sub-column masks of all columns of the current call
    DevBuf mask;
    DevBuf d_rnd;              // one slab of Mersenne-Twister deviates (irng = 1)
    bool batch_set = false; // rrtmg_lw_hip_set_batch has named a size (otherwise: auto_batch(nlay))
    int batch = DEFAULT_BATCH;     // columns per internal batch: 0.06-0.16 MB of workspace per column at 72 layers by call shape (38 GB of the 288 for the benchmark's); measured per 1e6 cloudy columns (end of round 2): 131072: 63.1 ms, 262144: 62.7, 524288: 61.7-62.3, 1048576: 61.2 - within the run-to-run spread, not worth the memory
    bool split_sweep = false;    // run the sweeps / k_flux of batch i concurrently with k_layer of batch i+1 (device entries).  Off by default: a sweep
                                 // workgroup owns a CU (transmittance table in LDS), so the two do not share a CU (measured: 1-2 % gain for twice the code scratch)
    bool sweep_attrs = false;    // the sweeps' dynamic-LDS limit has been raised on this device
    bool n1 = false;             // rrtmg_lw_hip_set_n1_prototype(1): cloud-free calls take the north-star-mapping prototype k_n1 (measurement only)
    // host-entry staging
    DevBuf stage_buf;
    // the *_as entries' staging: a batch's arrays in float64 reference form; play, cldfr, alpha of a whole fused McICA call for the generator
    DevBuf form_buf, form_gen;
    Stream stream;
    Stream cp_in, cp_out;                               // host-pointer entries: H2D and D2H copy streams
    PinnedBuf h_tot;                                    // pinned host scratch of the non-McICA host entry: tauctot of HOST_SETS column batches
    // pinned host staging of the host-pointer entries, HOST_SETS sets like the device staging: `in` = the rows of the caller's PAGEABLE input
    // arrays that travel (packed by the host threads, then one DMA per run of rows), `out` = the pageable output arrays' rows (DMA, then
    // unpacked by the host threads), `fill` = the table of k_fill_rows (rows that do not travel); the *_r4 entries: `widen` / `narrow` =
    // the tables of k_widen_rows (float32 input rows that have landed) and k_narrow_rows (the active output rows)
    struct HostSet { PinnedBuf in, out, fill, widen, narrow; } hset[HOST_SETS];
    Event ev_h2d[HOST_SETS], ev_cmp[HOST_SETS], ev_d2h[HOST_SETS];
    KissTable kiss;             // the kissvec generator's jump tables of the last KISS_SLOTS (draws per sub-column, permuteseed) pairs, on this device
    std::string err;
    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg)
    bool profile = false;
    // small device-resident calls replayed as ONE graph (run_pipelined): what a call's launches depend on -> the instantiated graph
    struct GraphEnt { std::vector<unsigned char> key; GraphExec exec; int seen = 0; bool failed = false; unsigned long long used = 0; };
    std::vector<GraphEnt> graphs;
    unsigned long long graph_clock = 0;
    Stream cap;                        // the stream the launches of such a call are captured on (the caller's may be the null stream)
    long long graph_replays = 0, graph_captures = 0;
    unsigned long long init_gen = 0;   // which initialisation (init_state) the state's tables come from: part of every graph's key
    struct ProfRec { const char *name; Event a, b; };
    std::vector<ProfRec> prof;
    std::vector<Event> evpool;          // events of finished profile records, handed out again by get_event()
};
// One State per device the library drives (rrtmg_lw_hip_init: one; rrtmg_lw_hip_init_devices: several GPUs from one process, SURVEY.md 8b
// `ndev`).  Every function below works on the calling thread's CURRENT state `G`: state 0 for every entry, and inside the host-pointer
// entries each worker thread of the fan-out (nomcica_host) takes the state of the device it feeds.  The same physical device may appear
// in several states ("virtual devices": separate workspaces, streams and table copies - how the fan-out is tested on a one-GPU box).
// The states, the queue (Q) and the generator's caches (g_mt) live in owned::NoDestroy storage: a process that ends without
// rrtmg_lw_hip_finalize - Python tests and host models do - must not call into the HIP runtime from static destructors, after the runtime
// may have been torn down.  finalize_state is the only path that releases them.
constexpr int MAXDEV = 16;
owned::NoDestroy<std::array<State, MAXDEV>> g_states_store;
std::array<State, MAXDEV> &g_states = g_states_store.get();
int g_ndev = 1;
thread_local State *g_cur = &g_states[0];
#define G (*g_cur)
std::mutex g_mu;

// ---- a GCM call below the C entry points --------------------------------------------------------------------------------------------
// An extern "C" entry fills these once and everything beneath takes them.  The arrays travel in the structs of kernels.hip - GcmIn (the
// McICA entries: its six cloud members null, McIn beside it), FluxOut with the spectral four, the generator's alpha as a plain pointer
// beside them - whether they hold the caller's host pointers (above the staging layer) or device pointers.
struct CallDesc {
    int ncol, nlay;
    int *icld;                                    // in / out: the entries write back the value they clamp it to
    int idrv, inflg, iceflg, liqflg;
    int permuteseed = 0; int *irng = nullptr;     // the fused generator + solver entries
    bool spectral = false;                        // a *_spectral entry: uflxs and dflxs are required (check_spec)
    size_t esz = 8;                               // bytes per element of the caller's HOST arrays: 4 in the *_r4 entries, whose float arrays travel in
                                                  // GcmIn / FluxOut as addresses only (nothing above the staging layer reads through them)
    int ld = 0;                                   // the *_view entries: columns between two rows of the caller's column-fastest device arrays (0: ncol)
};
CallDesc real4(CallDesc d) { d.esz = 4; return d; }
CallDesc spectral(CallDesc d) { d.spectral = true; return d; }
CallDesc strided(CallDesc d, int ld) { d.ld = ld; return d; }

// The scalars of a batch below the entry points, as CallDesc and the array structs are for a call: what is fixed for the call, and the
// columns [col0, col0 + nb) of arrays nct columns wide that one batch takes, out of the ncall columns of the call (the arrays of a *_view
// call are wider than the call: nct = ld >= ncall, every pointer at the call's first column).  Whoever knows the values names them once; run_prep,
// run_layer, run_sweep, run_batch and run_optics read them.
struct Batch {
    int nlay = 0, nct = 0, ncall = 0;
    int mode = 0;                                 // 0 clear, 1 rtrn, 2 rtrnmr, 3 rtrnmc (McICA)
    int idrv = 0;
    int istart = 1, iend = 16;                    // only bands in [istart, iend] (the column entries)
    int inflag = 0, iceflag = 0, liqflag = 0;
    const McIn *mc = nullptr;                     // mode 3: the sub-column arrays, or null when the sub-columns come from the generator's mask (Workspace::mask)
    int nb = 0, col0 = 0;                         // this batch
    int acc = 0, nsamp = 1, isamp = 0;            // a sample (isamp = 0 .. nsamp - 1) of a call that averages nsamp of them (run_samples): 0 k_flux stores, 1 adds, 2 adds and divides
    int share = 0;                                // ... 1: k_layer leaves the cells' float64 optical depths in W.odg (the first sample), 2: k_codet forms the
                                                  // sample's total codes from them and k_layer does not run (a later sample of the same batch)
};
// a GCM call's batches: all bands, arrays as wide as the call - or, in a *_view call, as its `ld` says
Batch batch_of(const CallDesc &d, int mode, const McIn *mc = nullptr)
{
    Batch b;
    b.nlay = d.nlay; b.nct = d.ld > 0 ? d.ld : d.ncol; b.ncall = d.ncol; b.mode = mode; b.idrv = d.idrv;
    b.inflag = d.inflg; b.iceflag = d.iceflg; b.liqflag = d.liqflg; b.mc = mc;
    return b;
}
// ... and one of nb columns of its own, staged at column 0 (the host-pointer entries, the array-form entries)
Batch staged_batch(const CallDesc &d, int mode, int nb, const McIn *mc = nullptr)
{
    Batch b = batch_of(d, mode, mc);
    b.nct = b.ncall = b.nb = nb;
    return b;
}

// The arrays of a call by position: the inputs in rrtmg_lw's order (what "argument %d" of a refusal counts), the generator's alpha, the
// outputs.  A list of a call's pointers (gcm_pointers, flux_pointers) is indexed by these and by nothing else.
enum ArrayPos {
    A_PLAY, A_PLEV, A_TLAY, A_TLEV, A_TSFC, A_H2OVMR, A_O3VMR, A_CO2VMR, A_CH4VMR, A_N2OVMR, A_O2VMR, A_CFC11VMR, A_CFC12VMR, A_CFC22VMR,
    A_CCL4VMR, A_EMIS, A_CLDFR, A_TAUCLD, A_CICEWP, A_CLIQWP, A_REICE, A_RELIQ, A_TAUAER, A_ALPHA,
    A_UFLX, A_DFLX, A_HR, A_UFLXC, A_DFLXC, A_HRC, A_DUFLX_DT, A_DUFLXC_DT, A_UFLXS, A_DFLXS, A_UFLXCS, A_DFLXCS, NA_CALL,
    NA_GCM = A_ALPHA,       // rrtmg_lw's input arrays
    NA_IN = A_UFLX          // ... and alpha
};
// every array is [rows][ncol][inner] with rows = per_layer x nlay + extra; cloud: inatm reads it only when icld >= 1 (:893-910)
struct ArrayShape { size_t inner, per_layer, extra; bool cloud; };
constexpr ArrayShape CALL_ARRAYS[NA_CALL] = {
    {1, 1, 0, false}, {1, 1, 1, false}, {1, 1, 0, false}, {1, 1, 1, false}, {1, 0, 1, false},                      // play plev tlay tlev tsfc
    {1, 1, 0, false}, {1, 1, 0, false}, {1, 1, 0, false}, {1, 1, 0, false}, {1, 1, 0, false}, {1, 1, 0, false},  // h2o o3 co2 ch4 n2o o2
    {1, 1, 0, false}, {1, 1, 0, false}, {1, 1, 0, false}, {1, 1, 0, false}, {1, 0, 16, false},                     // cfc11 cfc12 cfc22 ccl4, emis (ncol,16)
    {1, 1, 0, true}, {NBND, 1, 0, true}, {1, 1, 0, true}, {1, 1, 0, true}, {1, 1, 0, true}, {1, 1, 0, true},     // cldfr taucld (16,ncol,nlay) cicewp cliqwp reice reliq
    {1, 16, 0, false}, {1, 1, 0, true},                                                                            // tauaer (ncol,nlay,16), alpha
    {1, 1, 1, false}, {1, 1, 1, false}, {1, 1, 0, false}, {1, 1, 1, false}, {1, 1, 1, false}, {1, 1, 0, false},  // uflx dflx hr uflxc dflxc hrc
    {1, 1, 1, false}, {1, 1, 1, false},                                                                            // duflx_dt duflxc_dt
    {1, 16, 16, false}, {1, 16, 16, false}, {1, 16, 16, false}, {1, 16, 16, false}};                               // the spectral four (ncol,nlay+1,16)
size_t rows_of(int a, size_t L) { return CALL_ARRAYS[a].per_layer * L + CALL_ARRAYS[a].extra; }

void gcm_pointers(const GcmIn &g, const double *alpha, const double *(&p)[NA_IN])
{
    p[A_PLAY] = g.play; p[A_PLEV] = g.plev; p[A_TLAY] = g.tlay; p[A_TLEV] = g.tlev; p[A_TSFC] = g.tsfc; p[A_H2OVMR] = g.h2ovmr;
    p[A_O3VMR] = g.o3vmr; p[A_CO2VMR] = g.co2vmr; p[A_CH4VMR] = g.ch4vmr; p[A_N2OVMR] = g.n2ovmr; p[A_O2VMR] = g.o2vmr;
    p[A_CFC11VMR] = g.cfc11vmr; p[A_CFC12VMR] = g.cfc12vmr; p[A_CFC22VMR] = g.cfc22vmr; p[A_CCL4VMR] = g.ccl4vmr; p[A_EMIS] = g.emis;
    p[A_CLDFR] = g.cldfr; p[A_TAUCLD] = g.taucld; p[A_CICEWP] = g.cicewp; p[A_CLIQWP] = g.cliqwp; p[A_REICE] = g.reice;
    p[A_RELIQ] = g.reliq; p[A_TAUAER] = g.tauaer; p[A_ALPHA] = alpha;
}
GcmIn gcm_from(const double *const *p)          // p[A_PLAY .. A_TAUAER]
{
    return GcmIn{p[A_PLAY], p[A_PLEV], p[A_TLAY], p[A_TLEV], p[A_TSFC], p[A_H2OVMR], p[A_O3VMR], p[A_CO2VMR], p[A_CH4VMR], p[A_N2OVMR],
                 p[A_O2VMR], p[A_CFC11VMR], p[A_CFC12VMR], p[A_CFC22VMR], p[A_CCL4VMR], p[A_EMIS], p[A_CLDFR], p[A_TAUCLD], p[A_CICEWP],
                 p[A_CLIQWP], p[A_REICE], p[A_RELIQ], p[A_TAUAER]};
}
void flux_pointers(const FluxOut &o, double *(&p)[NA_CALL])          // fills p[A_UFLX .. A_DFLXCS]
{
    p[A_UFLX] = o.uflx; p[A_DFLX] = o.dflx; p[A_HR] = o.hr; p[A_UFLXC] = o.uflxc; p[A_DFLXC] = o.dflxc; p[A_HRC] = o.hrc;
    p[A_DUFLX_DT] = o.duflx_dt; p[A_DUFLXC_DT] = o.duflxc_dt;
    p[A_UFLXS] = o.uflxs; p[A_DFLXS] = o.dflxs; p[A_UFLXCS] = o.uflxcs; p[A_DFLXCS] = o.dflxcs;
}
FluxOut flux_from(double *const *p)
{
    return FluxOut{p[A_UFLX], p[A_DFLX], p[A_HR], p[A_UFLXC], p[A_DFLXC], p[A_HRC], p[A_DUFLX_DT], p[A_DUFLXC_DT], nullptr, nullptr,
                   p[A_UFLXS], p[A_DFLXS], p[A_UFLXCS], p[A_DFLXCS]};
}
bool have_outs(const FluxOut &o) { return o.uflx && o.dflx && o.hr && o.uflxc && o.dflxc && o.hrc; }

// aggregation of small calls (rrtmg_lw_hip_queue_*): recorded chunks and the pinned staging set they are packed into
struct QueuedChunk { CallDesc d; GcmIn in; const double *alpha; FluxOut out; };       // alpha: the generator's (fused McICA calls; optional)
struct ChunkQueue {
    bool open = false;
    int nlay = 0, icld = 0, idrv = 0, inflg = 0, iceflg = 0, liqflg = 0;
    long long ncol = 0;
    std::vector<QueuedChunk> chunks;
    PinnedBuf pinned;
};
owned::NoDestroy<ChunkQueue> g_queue_store;       // (never destroyed: see g_states)
ChunkQueue &Q = g_queue_store.get();

// The HIP current device is per host thread: an entry called from another thread (an OpenMP host model, a Python worker) must
// select the device the workspace lives on, and leaves the caller's device selection as it found it.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    DeviceGuard()
    {
        if (G.init && hipGetDevice(&prev) == hipSuccess && prev != G.device) switched = hipSetDevice(G.device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define ENTRY_LOCK std::lock_guard<std::mutex> lk(g_mu); DeviceGuard dg_

// Device-pointer entries: the state (rrtmg_lw_hip_init_devices) of the device the caller's arrays live on, found from the first array
// (hipPointerGetAttributes) - a one-process host with device-resident data on several GPUs uses all of them through the same entries.
// Several states on ONE device (the virtual devices of the tests) take such calls in turn.  A pointer the runtime does not know keeps
// the first state (the behaviour until round 5); arrays on a device the library was not initialised for are an error.  g_cur is
// thread-local: put back when the entry returns.
thread_local int tl_dev_state = 0;          // the state this thread's last device-pointer entry ran on (rrtmg_lw_hip_last_device_state)
struct StateSelect {
    State *keep;
    bool bad = false;
    int dev = -1;
    // first_only: work that lives on the first state whatever the arrays' device (the Mersenne-Twister generator: ONE stream over all columns
    // of a call, its jump-ahead tables on the first device) - arrays elsewhere are an error
    explicit StateSelect(const void *p, bool first_only = false) : keep(g_cur)
    {
        static unsigned turn = 0;
        tl_dev_state = 0;
        g_cur = &g_states[0];
        if (!p || g_ndev <= 1) return;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return; }
        dev = at.device;
        if (first_only) { bad = g_states[0].device != dev; return; }
        int match[16], n = 0;
        for (int d = 0; d < g_ndev && n < 16; d++) if (g_states[d].init && g_states[d].device == dev) match[n++] = d;
        if (n == 0) { bad = true; return; }
        tl_dev_state = match[turn++ % (unsigned)n];
        g_cur = &g_states[tl_dev_state];
    }
    ~StateSelect() { g_cur = keep; }
};
#define ENTRY_LOCK_FOR(ptr, ...) std::lock_guard<std::mutex> lk(g_mu); StateSelect ss_(ptr, ##__VA_ARGS__); DeviceGuard dg_; \
    if (ss_.bad) return fail(RRTMG_LW_HIP_EARG, "the arrays live on device %d, which the library was not initialised for (rrtmg_lw_hip_init_devices)", ss_.dev)

// The text of an error belongs to the THREAD whose call failed (concurrent callers: another thread's failure a moment later must not
// replace it before the caller has read it); the state keeps a copy for threads that have had no error of their own.
thread_local std::string tl_err;
// the library's latest error text whatever the thread, for a thread that has none of its own (rrtmg_lw_hip_last_error): under its own
// small lock, never the entry lock - a caller polling for errors must not wait out another thread's solve
std::mutex g_lasterr_mu;
std::string g_lasterr;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    G.err = buf;
    tl_err = buf;
    { std::lock_guard<std::mutex> lk(g_lasterr_mu); g_lasterr = buf; }
    return code;
}

#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// an owner's growth or release on a path that reports: the traits' code (a hipError_t) becomes the call's error
template <class Buf>
int grow(Buf &b, size_t need, size_t want, const char *what)
{
    if (const int e = b.reserve(need, want)) return fail(RRTMG_LW_HIP_EHIP, "%s: releasing the old buffer or allocating %zu bytes failed: %s", what, want, hipGetErrorString((hipError_t)e));
    return 0;
}
template <class Own>
int drop(Own &o, const char *what)
{
    if (const int e = o.reset()) return fail(RRTMG_LW_HIP_EHIP, "%s: release failed: %s", what, hipGetErrorString((hipError_t)e));
    return 0;
}
int make_event(Event &e) { HIP_TRY(hipEventCreateWithFlags(e.slot(), hipEventDisableTiming)); return 0; }

const char *physics_message(int code)
{
    switch (code) {   // texts of the reference's `stop` statements, src/rrtmg_lw_cldprop.f90:212,217,228,244,272
    case E_ICE_SMALL: return "ICE RADIUS TOO SMALL";
    case E_ICE_BOUNDS: return "ICE RADIUS OUT OF BOUNDS";
    case E_ICE_GEN_BOUNDS: return "ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS";
    case E_LIQ_BOUNDS: return "LIQUID EFFECTIVE RADIUS OUT OF BOUNDS";
    case E_BAD_FLAG: return "INVALID CLOUD PROPERTY FLAG";
    case E_MC_INFLAG1: return "INFLAG = 1 OPTION NOT AVAILABLE WITH MCICA";            // src/rrtmg_lw_cldprmc.f90:191
    case E_KISS_PMID: return "MCICA_SUBCOL: KISSVEC SEED GENERATOR REQUIRES PMID FROM BOTTOM FOUR LAYERS.";   // src/mcica_subcol_gen_lw.f90:465
    default: return "unknown physics error";
    }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the batch size in force for a call of nlay layers
int auto_batch(int nlay)
{
    if (nlay <= 96) return DEFAULT_BATCH;
    int b = DEFAULT_BATCH;
    while (b > 16384 && (long long)b * nlay > (long long)DEFAULT_BATCH * 72) b >>= 1;
    return b;
}
// The sweeps address the rows of a workspace array through a buffer descriptor built from the array's start (kernels.hip: sweep_rsrc,
// num_records = SWEEP_RANGE bytes) with the level's row as a 32-bit scalar byte offset (bload_*'s soff) and the column as the per-lane
// offset.  Every byte a sweep touches must lie inside the descriptor's range whatever the hardware's range check counts - the per-lane
// offset alone or the scalar offset with it (profiles/lifecycle_tests.md) - so a batch is halved until the END of the last row of
// the array with the largest rows does: rtrnmr's overlap factors, 3 rows of 16 bytes per column for each of the levels 0 .. nlay, i.e.
// (nlay + 1) x 48 bytes per column (262 144 columns: beyond 169 layers).  The other arrays read this way stay below it in every mode: the
// sub-column cloud fractions / emissivities of rtrnmc nlay x 32 bytes per column, the cell codes nlay x 16, rtrn's emissivity term
// nlay x 8, the cloud flags (nlay + 2) x 4, the binary-key words nlay x 4.  The default batches (auto_batch) are far inside:
// 72 layers x 262 144 columns end at 0.43 of the range, 137 x 131 072 at 0.40, 200 x 65 536 at 0.29.
constexpr unsigned long long SWEEP_RANGE = 0x7ffffff0ull;
int eff_batch(int nlay)
{
    int b = G.batch_set ? G.batch : auto_batch(nlay);
    while (b > 64 && (unsigned long long)(nlay + 1) * 48ull * (unsigned long long)b > SWEEP_RANGE) b >>= 1;
    return b;
}
// columns per batch: the fewest batches that respect G.batch, of (nearly) equal size - a short last batch would leave the
// pipelines (prep / layer / sweep of neighbouring batches) unbalanced, e.g. 125000 columns -> 2 x 62720 rather than 65536 + 59464
int balanced_batch(int ncol, int cap)
{
    if (ncol <= cap) return ncol;
    const int nbatch = (ncol + cap - 1) / cap;
    const int nb = (int)align_up((size_t)(ncol + nbatch - 1) / nbatch, 256);
    return std::min(nb, cap);
}

Event get_event()
{
    Event e;
    if (!G.evpool.empty()) { e = std::move(G.evpool.back()); G.evpool.pop_back(); }
    else (void)hipEventCreate(e.slot());
    return e;
}

// launch wrapper: brackets the kernel with events when profiling is on
#define LAUNCH(NAME, KERNEL, GRID, BLOCKDIM, STREAM, ...)                                        \
    do {                                                                                         \
        if (G.profile) {                                                                         \
            State::ProfRec r_{NAME, get_event(), get_event()};                                   \
            (void)hipEventRecord(r_.a.get(), STREAM);                                            \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCKDIM, 0, STREAM, __VA_ARGS__);                  \
            (void)hipEventRecord(r_.b.get(), STREAM);                                            \
            G.prof.push_back(std::move(r_));                                                     \
        } else {                                                                                 \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCKDIM, 0, STREAM, __VA_ARGS__);                  \
        }                                                                                        \
    } while (0)

// the same with dynamic LDS
#define LAUNCH_LDS(NAME, KERNEL, GRID, BLOCKDIM, LDS, STREAM, ...)                               \
    do {                                                                                         \
        if (G.profile) {                                                                         \
            State::ProfRec r_{NAME, get_event(), get_event()};                                   \
            (void)hipEventRecord(r_.a.get(), STREAM);                                            \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCKDIM, LDS, STREAM, __VA_ARGS__);                \
            (void)hipEventRecord(r_.b.get(), STREAM);                                            \
            G.prof.push_back(std::move(r_));                                                     \
        } else {                                                                                 \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCKDIM, LDS, STREAM, __VA_ARGS__);                \
        }                                                                                        \
    } while (0)

// after the launches of a batch's stage
int launches_ok()
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- which kernel instantiations there are ------------------------------------------------------------------------------------------
// The sweeps (k_sweepc, k_sweepz) and k_layer are templates over what a call's shape decides.  Per family ONE predicate says which
// combinations are instantiated and ONE dispatcher turns the run-time choice into compile-time constants; raising the sweeps' LDS limit
// (ensure_sweep_attrs) and launching them (run_sweep) both go through the dispatcher, so an instantiation is added in these two places.
// Tuning builds (tools/build_variant.sh name -DRRLW_TUNE ...): only the kernels of the benchmark's default workload - GCM entry,
// rtrn / rtrnmr, idrv = 0 - are instantiated (a quarter of the compile time); every other call shape is refused.
#ifdef RRLW_TUNE
constexpr bool TUNING = true;
#else
constexpr bool TUNING = false;
#endif
// Phase 1 (down, above the clouds) forms no d/dT terms: it has no d/dT instantiation, and a call with idrv = 1 launches its plain one.
constexpr bool sweepc_exists(int phase, bool ddt) { return !ddt || (!TUNING && phase != 1); }
constexpr bool sweepc_ddt(int phase, int idrv) { return idrv == 1 && phase != 1; }
constexpr bool sweepz_exists(int mode, bool ddt) { return !TUNING || (mode == 2 && !ddt); }
constexpr bool layer_exists(bool gcm, int cloud) { return TUNING ? gcm && cloud == 1 : gcm || cloud != 3; }     // the generator's mask: GCM entries only

// f(std::integral_constant<int, V>) for the V among Vs that v equals; v = EVERY: for each of them in turn, until one fails
constexpr int EVERY = -1;
template <int... Vs, class F>
int with_const(int v, F &&f)
{
    int rc = 0;
    bool hit = false;
    ((((v == Vs || v == EVERY) && rc == 0) ? (void)(hit = true, rc = f(std::integral_constant<int, Vs>{})) : (void)0), ...);
    return hit ? rc : fail(RRTMG_LW_HIP_EARG, "internal: no kernel instantiation for %d", v);
}

// the names the profile records carry (State::ProfRec::name): "k_sweepc<4,1>", "k_sweepz<3,2,spec>"
struct KernelName { char s[24]; };
constexpr KernelName sweep_name(char family, int nq, int x, bool spec)
{
    KernelName n{};
    int k = 0;
    for (const char *p = "k_sweep"; *p; p++) n.s[k++] = *p;
    n.s[k++] = family; n.s[k++] = '<'; n.s[k++] = (char)('0' + nq); n.s[k++] = ','; n.s[k++] = (char)('0' + x);
    if (spec) for (const char *p = ",spec"; *p; p++) n.s[k++] = *p;
    n.s[k++] = '>';
    return n;
}
// what a launch needs of an instantiation: its name, threads (waves) per band, column sub-blocks per workgroup for a group of nbands, LDS
template <int Q, int PH, bool I, bool SPEC>
struct SweepC {
    static constexpr KernelName name = sweep_name('c', Q, PH, SPEC);
    static constexpr int nt = sweepc_nt(Q, PH);
    static constexpr auto kernel() { return &k_sweepc<Q, PH, I, nt, SPEC>; }
    static int nsb(int nbands) { return sweepc_nsb(Q, PH, I, nbands); }
    static int lds_bytes(int wnb, int nsb) { return sweepc_lds_bytes(PH, I, wnb, nsb, nt); }
};
template <int Q, int M, bool I, bool SPEC>
struct SweepZ {
    static constexpr KernelName name = sweep_name('z', Q, M, SPEC);
    static constexpr int nt = sweepz_nt(Q);
    static constexpr auto kernel() { return &k_sweepz<Q, M, I, SPEC>; }
    static int nsb(int nbands) { return sweepz_nsb(Q, nbands, I); }
    static int lds_bytes(int wnb, int nsb) { return sweepz_lds_bytes(wnb, nsb, nt, I); }
};
// k_sweepc of bands of nq quads, phase 0 (a whole cloud-free column) / 1 (down, above the clouds) / 2 (up, above the clouds), with d/dT
// terms or not, with spectral outputs or not: f(SweepC<..>{}).  EVERY for all four: f for every instantiation there is.
template <class F>
int sweepc_dispatch(int nq, int phase, int ddt, int spec, F &&f)
{
    return with_const<1, 2, 3, 4>(nq, [&](auto Q) { return with_const<0, 1, 2>(phase, [&](auto PH) {
           return with_const<0, 1>(ddt, [&](auto I) { return with_const<0, 1>(spec, [&](auto S) {
               if constexpr (sweepc_exists(decltype(PH)::value, decltype(I)::value != 0))
                   return f(SweepC<decltype(Q)::value, decltype(PH)::value, decltype(I)::value != 0, decltype(S)::value != 0>{});
               else return ddt == EVERY ? 0 : fail(RRTMG_LW_HIP_EARG, "internal: no such k_sweepc");
           }); }); }); });
}
// k_sweepz (the cloud zone) of bands of nq quads, mode 1 rtrn / 2 rtrnmr / 3 rtrnmc with sub-column arrays / 4 rtrnmc with the generator's mask
template <class F>
int sweepz_dispatch(int nq, int mode, int ddt, int spec, F &&f)
{
    return with_const<1, 2, 3, 4>(nq, [&](auto Q) { return with_const<1, 2, 3, 4>(mode, [&](auto M) {
           return with_const<0, 1>(ddt, [&](auto I) { return with_const<0, 1>(spec, [&](auto S) {
               if constexpr (sweepz_exists(decltype(M)::value, decltype(I)::value != 0))
                   return f(SweepZ<decltype(Q)::value, decltype(M)::value, decltype(I)::value != 0, decltype(S)::value != 0>{});
               else return ddt == EVERY ? 0 : fail(RRTMG_LW_HIP_EARG, "internal: no such k_sweepz");
           }); }); }); });
}

constexpr int N1_LDS_MAX = 160 * 1024;      // the prototype k_n1 (run_sweep, G.n1)
// the sweeps stage the transmittance table in LDS: more than the 64 KB a kernel may use without asking.  Per device, once.
int ensure_sweep_attrs()
{
    if (G.sweep_attrs) return 0;
    const auto raise = [](auto K) { HIP_TRY(hipFuncSetAttribute((const void *)K.kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, SWEEPC_LDS_MAX)); return 0; };
    if (int rc = sweepc_dispatch(EVERY, EVERY, EVERY, EVERY, raise)) return rc;
    if (int rc = sweepz_dispatch(EVERY, EVERY, EVERY, EVERY, raise)) return rc;
    // (k_flux: its exchange tile, flux_lds_bytes, is static and far below 64 KB)
#ifndef RRLW_TUNE
    HIP_TRY(hipFuncSetAttribute((const void *)k_n1<false>, hipFuncAttributeMaxDynamicSharedMemorySize, N1_LDS_MAX));      // (the prototype run_sweep launches when G.n1 is set)
#endif
    G.sweep_attrs = true;
    return 0;
}

// The sweeps' band groups: the bands in [istart, iend] by their number of quads, at most as many per group as one sweep workgroup holds
// (a group is one workgroup in k_sweepc and in k_sweepz: what fits the wave slots of both).  Every group has its own partial slabs.
struct SweepGroups { int n = 0; int nb[NGROUP_MAX]; unsigned long long bands[NGROUP_MAX]; int gq[NGROUP_MAX]; };
bool make_groups(int mode, int idrv, int istart, int iend, SweepGroups &fg)
{
    unsigned long long lists[5] = {0, 0, 0, 0, 0};
    int nbs[5] = {0, 0, 0, 0, 0};
    for (int nq = 1; nq <= 4; nq++)
        for (int B = 1; B <= NBND; B++)
            if (band_nquad(B) == nq && B >= istart && B <= iend) lists[nq] |= (unsigned long long)(B - 1) << (4 * nbs[nq]++);
    fg.n = 0;
    for (int nq = 4; nq >= 1; nq--) {
        const int zcap = sweepz_group_cap(nq, idrv == 1);
        const int cap = std::max(1, std::min(sweepc_group_cap(nq), mode != 0 ? zcap : 99));
        for (int k0 = 0; k0 < nbs[nq]; k0 += cap) {
            if (fg.n >= NGROUP_MAX) return false;
            const int nbg = std::min(cap, nbs[nq] - k0);
            fg.nb[fg.n] = nbg;
            fg.bands[fg.n] = (lists[nq] >> (4 * k0)) & (nbg >= 16 ? ~0ull : ((1ull << (4 * nbg)) - 1ull));
            fg.gq[fg.n++] = nq;
        }
    }
    return true;
}

// (re)allocate the per-batch workspace.  It holds what the call shapes seen so far need and grows with them: the partial slabs of as many
// band groups as the sweeps form (4 without d/dT, up to NGROUP_MAX with), the d/dT slab only for idrv = 1, rtrn's / rtrnmc's emissivity
// term only for modes 1 and 3, rtrnmr's overlap factors only for mode 2.  mode: 0 clear, 1 rtrn, 2 rtrnmr, 3 rtrnmc; -1 = everything.
void graphs_clear();      // (the graphs of small calls hold workspace addresses)
// Batches of up to this many columns are swept ONE band per workgroup (SweepArgs::split; rrtmg_lw_hip_set_split_max / RRTMG_LW_SPLIT_MAX):
// 1 024 columns are 16 blocks of 64 - as groups of bands 16 workgroups of twelve waves on 16 of the 256 CUs, as single bands 256
// workgroups of one to four waves on all of them.  A level of a sweep then costs the dependent issue of ONE wave per SIMD instead of
// three; results bit-identical (k_flux adds a group's bands first).  0 = never.
// Default 768: sixteen bands x twelve blocks = 192 workgroups, each of which wants a CU to itself (the transmittance table takes half of the
// LDS) - at 1 024 columns the 256 workgroups no longer all find one at once, some wait for a second round and the gain is gone; at 4 096
// the rounds make the sweeps 1.6 x slower (profiles/round5_small_calls.md).
int g_split_max = []() { const char *e = getenv("RRTMG_LW_SPLIT_MAX"); return e ? std::max(0, atoi(e)) : 768; }();
int ensure_workspace(int nlay, int ncolb, bool cloud, bool mc = false, int idrv = 1, int mode = -1)
{
    SweepGroups fgw;
    int groups = NGROUP_MAX;
    if (mode >= 0 && make_groups(mode, idrv, 1, NBND, fgw)) groups = fgw.n;
    const bool gdp = idrv == 1, efcl = cloud && (mode < 0 || mode == 1 || mode == 3), ovl = cloud && (mode < 0 || mode == 2);
    // (a batch small enough for the split sweeps - one band per workgroup, a slab per band - needs room for sixteen slabs of its own width)
    const size_t split_cols = ncolb <= g_split_max ? (size_t)NBND * align_up((size_t)ncolb, 64) : 0;
    const State::WsShape &have = G.ws;         // (stays until the new workspace stands: what earlier call shapes needed is merged into it)
    if (G.ws_buf && have.nlay == nlay && have.ncolb >= ncolb && (have.cloud || !cloud) && (have.mc || !mc) && (have.two_scr || !G.split_sweep) &&
        have.groups >= groups && have.slabcols >= split_cols && (have.gdp || !gdp) && (have.efcl || !efcl) && (have.ovl || !ovl)) return 0;
    if (G.ws_buf) { HIP_TRY(hipDeviceSynchronize()); graphs_clear(); if (int rc = drop(G.ws_buf, "workspace")) return rc; }
    const bool same = have.nlay == nlay;
    ncolb = std::max(ncolb, same ? have.ncolb : 0);
    cloud = cloud || have.cloud || mc;
    mc = mc || have.mc;
    const int ng = std::max(groups, have.groups);
    const bool want_gdp = gdp || have.gdp, want_efcl = efcl || have.efcl, want_ovl = ovl || have.ovl;
    const size_t n = (size_t)ncolb, L = (size_t)nlay;
    const size_t slabcols = std::max((size_t)ng * n, (size_t)NBND * align_up(std::min(n, (size_t)std::max(g_split_max, 0)), 64));
    struct Item { void **p; size_t bytes; };
    Workspace &W = G.W;
    W = Workspace{};
    std::vector<Item> items = {
        {(void **)&W.gdn1, slabcols * (L + 1) * sizeof(double)},
        {(void **)&W.gup1, slabcols * (L + 1) * sizeof(double)},
        {(void **)&W.gup, slabcols * (L + 1) * sizeof(Part2)},
        {(void **)&W.gdn, slabcols * (L + 1) * sizeof(Part2)},
    };
    if (want_gdp) items.push_back({(void **)&W.gdp, slabcols * (L + 1) * sizeof(Part2)});
    const bool two_scr = G.split_sweep;
    G.scrset[1] = State::ScrSet{};
    for (int k = 0; k < (two_scr ? 2 : 1); k++) {
        State::ScrSet &ss = G.scrset[k];
        ss = State::ScrSet{};
        items.push_back({(void **)&ss.scr[S_CODE], (size_t)NQUAD * L * n * CODE_BYTES});
        items.push_back({(void **)&ss.fw, (size_t)NFW * L * n * sizeof(unsigned)});
        if (cloud) items.push_back({(void **)&ss.scr[S_CODET], (size_t)NQUAD * L * n * CODE_BYTES});
    }
    for (auto &ps : G.prep) {
        ps = State::PrepSet{};
        items.push_back({(void **)&ps.percol, (size_t)NPERCOL * n * 8});
        items.push_back({(void **)&ps.laytrop, n * 4});
        items.push_back({(void **)&ps.ncbands, n * 4});
        items.push_back({(void **)&ps.cflag, (L + 2) * n * 4});
        const size_t nblk = (n + 63) / 64, nslot = (size_t)sort_slots((int)nblk);
        items.push_back({(void **)&ps.btop, nblk * 4});
        items.push_back({(void **)&ps.hblk, nblk * 4});
        items.push_back({(void **)&ps.order, nslot * 4});
        items.push_back({(void **)&ps.hgrp, (nslot / SORT_GROUP) * 4});
        items.push_back({(void **)&ps.bbot, nblk * 4});
        items.push_back({(void **)&ps.hbot, (nslot / SORT_GROUP) * 4});
        items.push_back({(void **)&ps.perm, align_up(n, COLSORT_WIN) * 4});
        items.push_back({(void **)&ps.wsort, (align_up(n, COLSORT_WIN) / COLSORT_WIN) * 4});
        items.push_back({(void **)&ps.wide, (2 + ((n + LAYER_BLOCK - 1) / LAYER_BLOCK) * L) * 4});
        if (cloud) {        // (reordered windows: the temperature and cloud-fraction rows of the caller once more, in position order)
            items.push_back({(void **)&ps.tlayc, L * n * 8});
            items.push_back({(void **)&ps.tlevc, (L + 1) * n * 8});
            items.push_back({(void **)&ps.cldfc, L * n * 8});
        }
    }
    if (cloud) items.push_back({(void **)&W.hand, (size_t)5 * NQUAD * 4 * n * 8});
    if (cloud) {
        for (auto &ps : G.prep) {
            items.push_back({(void **)&ps.odcld, 16 * L * n * 8});
            if (want_efcl) items.push_back({(void **)&ps.efcl, 16 * L * n * 8});
            if (want_ovl) items.push_back({(void **)&ps.ovl, (size_t)2 * (L + 1) * 3 * n * sizeof(double2)});
        }
    }
    if (mc) {
        items.push_back({(void **)&W.odg, (size_t)NQUAD * 4 * L * n * 8});
        items.push_back({(void **)&W.cfef, (size_t)NQUAD * 8 * L * n * 4});
    }
    size_t total = 0;
    for (auto &it : items) total += align_up(it.bytes, 256);
    if (int rc = grow(G.ws_buf, total, total, "workspace")) return rc;
    size_t off = 0;
    for (auto &it : items) { *it.p = G.ws_buf.as<char>() + off; off += align_up(it.bytes, 256); }
    for (auto &ps : G.prep) HIP_TRY(hipMemset(ps.wide, 0, 8));         // the count of k_layer's wide-window list (kernels.hip: k_layer)
    W.ncolb = ncolb;
    W.pcb = ncolb;
    W.nlay = nlay;
    W.err = G.d_err.as<int>();
    for (int a = 0; a < NSCR; a++) W.scr[a] = G.scrset[0].scr[a];
    W.fw = G.scrset[0].fw;
    {   // G.W itself carries prep set 0 and scratch set 0
        const State::PrepSet &ps = G.prep[0];
        W.percol = ps.percol; W.laytrop = ps.laytrop; W.ncbands = ps.ncbands; W.cflag = ps.cflag;
        W.odcld = ps.odcld; W.efcl = ps.efcl; W.ovl = ps.ovl;
        W.btop = ps.btop; W.order = ps.order; W.hgrp = ps.hgrp; W.hblk = ps.hblk; W.bbot = ps.bbot; W.hbot = ps.hbot;
    }
    G.ws = State::WsShape{nlay, ncolb, cloud, mc, want_gdp, want_efcl, want_ovl, two_scr, ng, slabcols};
    return 0;
}

int ensure_mask(int nlay, size_t ncol)
{
    const size_t bytes = (size_t)KJ_NWORD * nlay * ncol * sizeof(unsigned);
    return grow(G.mask, bytes, bytes, "sub-column masks");
}

// Columns of a cloudy non-McICA batch are taken in the order k_colsort gives them (by cloud top within windows of 256: the sweeps decide
// per 64 positions where the clouds end).  rrtmg_lw_hip_set_column_sort / RRTMG_LW_COLSORT=0 switch it off; results do not depend on it.
bool g_colsort = []() { const char *e = getenv("RRTMG_LW_COLSORT"); return !e || atoi(e) != 0; }();
bool use_colsort(bool gcm, int mode, int nb);
// block-levels a window's reordering must take out of the cloud zone (k_colsort; measured break-even on an MI355X, profiles/round4_column_order.md)
constexpr int COLSORT_NEVER = 1 << 24;     // no window gains this many block-levels (4 blocks x 603 layers at most): "never reorder"
int g_colsort_min = []() { const char *e = getenv("RRTMG_LW_COLSORT_MIN"); return e ? std::max(0, std::min(atoi(e), COLSORT_NEVER)) : 24; }();
// what a block that the reordering leaves without any cloud adds to its window's gain, in per cent of nlay block-levels (k_colsort's
// clear_bonus; rrtmg_lw_hip_set_column_sort_clear / RRTMG_LW_COLSORT_CLEAR; measurement: profiles/clear_groups.md)
constexpr int COLSORT_CLEAR_MAX = 1000;
constexpr int COLSORT_CLEAR_DEFAULT = 18;      // 12 block-levels at 72 layers: with the 13.8 the benchmark's windows gain on average, past the threshold of 24 (profiles/clear_groups.md)
int g_colsort_clear = []() { const char *e = getenv("RRTMG_LW_COLSORT_CLEAR"); return e ? std::max(0, std::min(atoi(e), COLSORT_CLEAR_MAX)) : COLSORT_CLEAR_DEFAULT; }();
// Block groups of a cloudy batch that hold no cloud (hand-off level 0) are swept as a cloud-free call sweeps its columns - one launch, one
// stream, 8-byte partials (SweepArgs::cfree, run_sweep).  rrtmg_lw_hip_set_clear_groups / RRTMG_LW_CLEAR_GROUPS=0 keep them in the three
// cloudy launches; results do not depend on it.
bool g_clear_groups = []() { const char *e = getenv("RRTMG_LW_CLEAR_GROUPS"); return !e || atoi(e) != 0; }();

// the workspace view of prep set k (see State::prep); sorted: the batch's columns go through k_colsort's order
Workspace ws_for(int k, bool sorted)
{
    Workspace w = G.W;
    const State::PrepSet &ps = G.prep[k];
    w.perm = sorted ? ps.perm : nullptr;
    w.wsort = sorted ? ps.wsort : nullptr;
    w.tlayc = ps.tlayc; w.tlevc = ps.tlevc; w.cldfc = ps.cldfc;
    w.wide = ps.wide;
    w.percol = ps.percol; w.laytrop = ps.laytrop; w.ncbands = ps.ncbands; w.cflag = ps.cflag;
    w.odcld = ps.odcld; w.efcl = ps.efcl; w.ovl = ps.ovl;
    w.btop = ps.btop; w.order = ps.order; w.hgrp = ps.hgrp; w.hblk = ps.hblk; w.bbot = ps.bbot; w.hbot = ps.hbot;
    const State::ScrSet &ss = G.scrset[G.ws.two_scr ? k : 0];
    for (int a = 0; a < NSCR; a++) w.scr[a] = ss.scr[a];
    w.fw = ss.fw;
    return w;
}

// A stream confined to the CUs [lo, hi) of the device's CU-mask order (hipExtStreamCreateWithCUMask; on a multi-XCD device consecutive
// mask bits go round the XCDs, so a run of bits that is a multiple of 8 long takes the same number of CUs from every XCD), or - lo = hi -
// an ordinary non-blocking stream.
int make_stream(Stream &st, int lo, int hi)
{
    if (hi <= lo) { HIP_TRY(hipStreamCreateWithFlags(st.slot(), hipStreamNonBlocking)); return 0; }
    uint32_t mask[32] = {};
    const int nw = (G.cu_total + 31) / 32;
    for (int b = lo; b < hi && b < 1024; b++) mask[b >> 5] |= 1u << (b & 31);
    HIP_TRY(hipExtStreamCreateWithCUMask(st.slot(), (uint32_t)nw, mask));
    return 0;
}
int ensure_sweep_set(int k)
{
    if (G.swset[k].q[0]) return 0;
    const int lo = k == 1 ? G.cu_layer : 0, hi = k == 1 ? G.cu_total : 0;
    State::SweepSet SS;         // (built here and moved in whole: a failure part-way leaves the state's set as it was)
    if (int rc = make_stream(SS.main, lo, hi)) return rc;
    for (int j = 0; j < 3; j++) {
        if (int rc = make_stream(SS.q[j], lo, hi)) return rc;
        if (int rc = make_event(SS.done[j])) return rc;
    }
    if (int rc = make_event(SS.go)) return rc;
    G.swset[k] = std::move(SS);
    return 0;
}

// A cloudy batch too small to fill the chip is a latency chain of six kernels; three of them are the sweeps (down above the clouds, the
// cloud zone, up above the clouds).  Up to ONE_SWEEP_MAX columns the cloud-zone kernel walks all levels instead (k_blocksort, force_top)
// and the two clear-sky launches are not made: 1 024 cloudy columns 0.609 -> 0.587 ms (profiles/round4_small_calls.md).  Larger batches keep the three launches - above the
// clouds k_sweepc costs a third of k_sweepz's clear-sky body per level.
int g_one_sweep_max = []() { const char *e = getenv("RRTMG_LW_ONE_SWEEP_MAX"); return e ? atoi(e) : 4096; }();       // rrtmg_lw_hip_set_one_sweep_max
bool one_sweep(int nb, int mode) { return mode != 0 && nb <= g_one_sweep_max; }
// k_layer's second pass with the wide staging window (terrain-following pressure grids; kernels.hip: StageWin).  rrtmg_lw_hip_set_wide_window /
// RRTMG_LW_WIDE_WINDOW=0 switch it off (measurement: every workgroup then keeps the narrow window, as before round 5); same results either way.
bool g_wide_window = []() { const char *e = getenv("RRTMG_LW_WIDE_WINDOW"); return !e || atoi(e) != 0; }();
// k_layer's bands of a (window, layer) over several workgroups where the batch does not fill the chip (run_layer).  rrtmg_lw_hip_set_layer_split /
// RRTMG_LW_LAYER_SPLIT=0.  Results do not depend on it.
bool g_prep_fork = []() { const char *e = getenv("RRTMG_LW_PREP_FORK"); return !e || atoi(e) != 0; }();     // (run_prep: k_colprep beside k_cloudscan; measurement switch)
bool g_layer_split = []() { const char *e = getenv("RRTMG_LW_LAYER_SPLIT"); return !e || atoi(e) != 0; }();
// (a batch that takes one sweep launch walks every level in the cloud-zone kernel whatever its blocks hold: nothing to gain from an order)
// (McICA, mode 3: with the generator's mask - the grid-mean cloud fraction gives the key; the sub-column ARRAYS of the reference's McICA
// argument list come without one and keep their order: the call sites pass `!mc`)
bool use_colsort(bool gcm, int mode, int nb) { return g_colsort && gcm && (mode == 1 || mode == 2 || mode == 3) && !one_sweep(nb, mode); }

// per-column part of one batch: k_colprep (+ k_cloudscan / k_cloudlay for rtrn / rtrnmr): it runs on the
// auxiliary stream one batch ahead of the heavy kernels (run_pipelined).
template <bool GCM>
int run_prep(hipStream_t s, const Workspace &Wk, const Batch &b, const GcmIn &g, const ColIn &c, hipStream_t side = nullptr)
{
    // thread-per-column kernels: one wave per workgroup so that a batch (one wave per 64 columns) spreads over all 256 CUs
    const dim3 cgrid1((b.nb + 63) / 64), cblock1(64);
    if (Wk.perm) {
        const dim3 wgrid((b.nb + COLSORT_WIN - 1) / COLSORT_WIN);
        LAUNCH("k_colsort", (k_colsort<GCM>), wgrid, dim3(COLSORT_WIN, COLSORT_TY), s, Wk, g, c, b.nb, b.col0, b.nct, g_colsort_min, (int)((long long)Wk.nlay * g_colsort_clear / 100));
    }
    // (k_cloudscan needs nothing of k_colprep - k_cloudlay does: the secants - and both are one dependent walk over a column's layers: with a
    // side stream, a call that is a single batch, they run side by side: -30 us of its 0.5 ms)
    const bool scan = b.mode == 1 || b.mode == 2, fork = scan && side && side != s;
    if (fork) {
        HIP_TRY(hipEventRecord(G.ev_fork.get(), s));
        HIP_TRY(hipStreamWaitEvent(side, G.ev_fork.get(), 0));
    }
    LAUNCH("k_colprep", (k_colprep<GCM>), cgrid1, cblock1, fork ? side : s, G.D, Wk, g, c, b.nb, b.col0, b.nct, b.idrv, b.istart, scan ? 0 : 1);
    if (fork) HIP_TRY(hipEventRecord(G.ev_join.get(), side));
    if (scan) {
        LAUNCH("k_cloudscan", (k_cloudscan<GCM>), cgrid1, cblock1, s, Wk, g, c, b.nb, b.col0, b.nct, b.inflag, b.iceflag, b.liqflag, b.mode);
        if (fork) HIP_TRY(hipStreamWaitEvent(s, G.ev_join.get(), 0));
        const dim3 lgrid((b.nb + BLOCK - 1) / BLOCK, Wk.nlay), lblock(BLOCK);
        LAUNCH("k_cloudlay", (k_cloudlay<GCM>), lgrid, lblock, s, G.D, Wk, g, c, b.nb, b.col0, b.nct, b.mode, b.inflag, b.iceflag, b.liqflag);
        LAUNCH("k_blocksort", k_blocksort, dim3(1), dim3(256), s, Wk, (b.nb + 63) / 64, one_sweep(b.nb, b.mode) ? 1 : 0);      // the blocks by cloud top, hand-off levels
    }
    return launches_ok();
}

// the arguments of a k_layer / k_optics launch over a batch's columns
LayerArgs layer_args(const Batch &b, const double *tauaer)
{
    LayerArgs la;
    la.ncol = b.nb; la.col0 = b.col0; la.nct = b.nct; la.idrv = b.idrv; la.istart = b.istart; la.iend = b.iend;
    la.ktab_bytes = (int)(G.H.ktab.size() * 8);
    la.tauaer = tauaer;
    const unsigned gx = (b.nb + LAYER_BLOCK - 1) / LAYER_BLOCK;
    // A batch whose (window, layer) pairs do not fill the chip - 768 workgroups at three per CU - spreads the bands of a pair over two or
    // four workgroups (k_layer: LayerArgs::partmask): a workgroup's sixteen bands are a 100 us chain, and a small call waits for ONE round
    // of them.  The parts follow the staging passes (a workgroup stages only the passes it has a band of).
    const auto bits = [](std::initializer_list<int> bands) { unsigned m = 0; for (int b : bands) m |= 1u << (b - 1); return m; };
    const unsigned quarter[4] = {bits({1, 2, 11, 15, 6}), bits({8, 10, 14, 16, 12, 13}), bits({4, 9, 7}), bits({3, 5})};
    const unsigned pairs_ = gx * (unsigned)b.nlay;
    la.nparts = !g_layer_split ? 1 : (pairs_ * 4 <= 1152 ? 4 : (pairs_ * 2 <= 1152 ? 2 : 1));
    for (int p = 0; p < 4; p++) la.partmask[p] = la.nparts == 4 ? quarter[p] : (la.nparts == 2 && p < 2 ? (quarter[2 * p] | quarter[2 * p + 1]) : 0xffffu);
    return la;
}

// layer-local part of one batch (k_cloudmc, k_layer), everything device-resident
template <bool GCM>
int run_layer(hipStream_t s, const Workspace &Wk, const Batch &b, const GcmIn &g, const ColIn &c)
{
    const dim3 block(BLOCK);
    if (b.mode == 3) {
        const dim3 cgrid((b.nb + BLOCK - 1) / BLOCK, b.nlay);
        if (b.mc) LAUNCH("k_cloudmc<arrays>", (k_cloudmc<false>), cgrid, block, s, G.D, Wk, *b.mc, g, b.nb, b.col0, b.nct, b.inflag, b.iceflag, b.liqflag);
        else LAUNCH("k_cloudmc<mask>", (k_cloudmc<true>), cgrid, block, s, G.D, Wk, McIn{}, g, b.nb, b.col0, b.nct, b.inflag, b.iceflag, b.liqflag);
        LAUNCH("k_blocksort", k_blocksort, dim3(1), dim3(256), s, Wk, (b.nb + 63) / 64, one_sweep(b.nb, b.mode) ? 1 : 0);
    }
    const LayerArgs la = layer_args(b, GCM ? g.tauaer : c.taua);
    const unsigned gx = (b.nb + LAYER_BLOCK - 1) / LAYER_BLOCK;
    const dim3 lgrid(gx, b.nlay, la.nparts), lblock(LAYER_BLOCK);
    // the wide-window pass over the (window, layer) pairs the narrow launch could not take (GCM entry; kernels.hip: StageWin): as many
    // workgroups as fit the chip at once, which leave at once when the list is empty
    Workspace Wn = Wk;
    if (!GCM || !HAVE_WIDE || !g_wide_window) Wn.wide = nullptr;
    const dim3 wgrid(gx * b.nlay, la.nparts);
    // (the list's count: cleared on the stream in front of the narrow launch - a memset node when the call is captured as a graph)
    if (Wn.wide) HIP_TRY(hipMemsetAsync(Wn.wide, 0, sizeof(int), s));
    if (b.share != 0) {         // an averaging call (run_samples): the gas optics of a batch once, a sample's total codes from them
        if constexpr (GCM && !TUNING) {
            if (b.mode != 3 || b.mc || !Wk.odg) return fail(RRTMG_LW_HIP_EARG, "internal: shared gas optics without the mask or the optical-depth array");
            if (b.share == 1) {
                LAUNCH("k_layer<mcshare,0>", (k_layer<true, CL_SHARE, 0>), lgrid, lblock, s, G.D, Wn, g, c, la);
                if (Wn.wide) LAUNCH("k_layer<mcshare,1>", (k_layer<true, CL_SHARE, 1>), wgrid, lblock, s, G.D, Wn, g, c, la);
            } else {
                LAUNCH("k_codet", k_codet, dim3((b.nb + BLOCK - 1) / BLOCK, b.nlay), block, s, G.D, Wk, b.nb, b.col0);
            }
            return launches_ok();
        } else return fail(RRTMG_LW_HIP_EARG, "shared gas optics: GCM entries only");
    }
    // k_layer's CLOUD: 0 clear, 1 cloud (rtrn / rtrnmr), 2 mcica (the sub-column arrays), 3 mcmask (the generator's mask)
    const int cloud = b.mode == 0 ? 0 : b.mode == 3 ? (b.mc ? 2 : 3) : 1;
    if (TUNING && !GCM) return fail(RRTMG_LW_HIP_EARG, "tuning build: GCM entry only");
    if (TUNING && cloud != 1) return fail(RRTMG_LW_HIP_EARG, "tuning build: cloudy non-McICA calls only");
    static const char *const names[4][2] = {{"k_layer<clear,0>", "k_layer<clear,1>"}, {"k_layer<cloud,0>", "k_layer<cloud,1>"},
                                            {"k_layer<mcica,0>", "k_layer<mcica,1>"}, {"k_layer<mcmask,0>", "k_layer<mcmask,1>"}};
    if (int rc = with_const<0, 1, 2, 3>(cloud, [&](auto CL) {
            constexpr int cl = decltype(CL)::value;
            if constexpr (layer_exists(GCM, cl)) {
                LAUNCH(names[cl][0], (k_layer<GCM, cl, 0>), lgrid, lblock, s, G.D, Wn, g, c, la);
                if constexpr (GCM) { if (Wn.wide) LAUNCH(names[cl][1], (k_layer<true, cl, 1>), wgrid, lblock, s, G.D, Wn, g, c, la); }
            }
            return 0;
        })) return rc;
    return launches_ok();
}

// what every sweep launch of a batch has in common (the group's bands, grid and slab come per launch)
template <bool GCM>
SweepArgs sweep_args(const Batch &b, const GcmIn &g, const ColIn &c, const FluxOut &out)
{
    SweepArgs sa{};
    sa.ncol = b.nb; sa.col0 = b.col0; sa.nct = b.nct; sa.idrv = b.idrv; sa.istart = b.istart; sa.iend = b.iend;
    sa.emis = GCM ? g.emis : c.semiss;
    sa.cldfrac = GCM ? g.cldfr : c.cldfrac;
    sa.tlay = GCM ? g.tlay : c.tavel;
    sa.tlev = GCM ? g.tlev : c.tz;
    // spectral outputs (GCM entries): the SPEC instantiations of the sweeps store every band's flux as well
    if (GCM && out.uflxs) { sa.uflxs = out.uflxs; sa.dflxs = out.dflxs; sa.uflxcs = out.uflxcs; sa.dflxcs = out.dflxcs; }
    return sa;
}

// vertical part of one batch: the sweep launches and k_flux
template <bool GCM>
int run_sweep(hipStream_t s, const Workspace &Wk_, const Batch &b, const GcmIn &g, const ColIn &c, const FluxOut &out, int sset = 0)
{
    Workspace Wk = Wk_;
    const int nb = b.nb;
    // a batch that does not fill the chip: one band per workgroup, a slab per band (g_split_max, SweepArgs::split) - where the slab arrays hold
    // sixteen slabs of the batch's width
    const size_t pcb_split = align_up((size_t)nb, 64);
    const bool split = nb <= g_split_max && (size_t)NBND * pcb_split <= G.ws.slabcols && pcb_split <= (size_t)Wk.ncolb;
    Wk.pcb = split ? (int)pcb_split : Wk.ncolb;
    if (int rc = ensure_sweep_attrs()) return rc;
    // The four sweep launches of a batch (bands of 4, 3, 2, 1 quads) are independent.  Each workgroup owns a CU, so a launch ends with
    // a partly filled last round (1-quad bands: 2.5 rounds); on separate streams the other launches' workgroups fill those CUs.
    // Measured: 10 000 columns 1.22 -> 0.98 ms; 125 000-column batches no gain (cloudy 98.9 -> 98.4 ms per 1e6 columns, McICA 115.5 -> 122.6).
    // (Round 3: for every batch size - 61.4 -> 60.2 ms per 1e6 cloudy columns, three runs each; deep clouds 87.7 -> 85.7.  The HIP-event
    // times of the sweep kernels then overlap: their sum exceeds the wall time they take together.)
    const bool fan = G.sweep_fanout;
    State::SweepSet &SS = G.swset[sset];
    if (fan) {
        if (int rc = ensure_sweep_set(sset)) return rc;
        HIP_TRY(hipEventRecord(SS.go.get(), s));
        for (int k = 0; k < 3; k++) HIP_TRY(hipStreamWaitEvent(SS.q[k].get(), SS.go.get(), 0));
    }
    SweepArgs sa = sweep_args<GCM>(b, g, c, out);
    const bool spec = sa.uflxs != nullptr;
#ifndef RRLW_TUNE
    if (G.n1 && b.mode == 0 && GCM && b.istart == 1 && b.iend == 16 && b.idrv == 0 && !spec && !out.uflx_var && !out.dflx_var && !out.hr_var && n1_lds_bytes(b.nlay) <= N1_LDS_MAX) {
        // prototype of the north-star mapping (one column per wavefront): replaces the sweeps, k_flux and k_rates of a cloud-free call
        // (it takes no spectral call)
        const dim3 ngrid((nb + N1_WAVES - 1) / N1_WAVES), nblock(64 * N1_WAVES);
        LAUNCH_LDS("k_n1", (k_n1<false>), ngrid, nblock, n1_lds_bytes(b.nlay), s, G.D, Wk, sa, out, g.plev);
        return launches_ok();
    }
#endif
    sa.split = split ? 1 : 0;
    // (cloud-free block groups of a batch that takes the three sweep launches: their own launch, below)
    const bool cfree = g_clear_groups && b.mode != 0 && !one_sweep(nb, b.mode);
    sa.cfree = cfree ? 1 : 0;
    // Per class of bands with the same number of quads: a cloud-free call (mode 0) is one k_sweepc<., 0> launch; the cloudy modes run
    // k_sweepc<., 1> (layers above the batch's highest cloud, downward), k_sweepz<., mode> (layers 1 .. ltop down, surface, up) and
    // k_sweepc<., 2> (layers above, upward).  The classes are independent of each other: with `fan` each class has its own stream;
    // on one stream the launches go phase by phase (all downward ones, then the cloud zone, then the upward ones) so that consecutive
    // launches never wait for each other's last workgroups.  With `cfree` a fourth launch per class, k_sweepc<., 0> over the sorted block
    // order, takes the groups that hold no cloud - whole columns, one stream - and the workgroups of the other three leave at once there
    // (each decides by its group's hand-off level; the grids stay those of the batch).
    SweepGroups fg;
    if (!make_groups(b.mode, b.idrv, b.istart, b.iend, fg)) return fail(RRTMG_LW_HIP_EARG, "internal: more than %d sweep groups", NGROUP_MAX);
    if ((!split && fg.n > G.ws.groups) || (b.idrv == 1 && !G.ws.gdp)) return fail(RRTMG_LW_HIP_EARG, "internal: workspace holds %d band groups, the call needs %d", G.ws.groups, fg.n);
    // first slab of every group, slabs per group (k_flux)
    int slab0[NGROUP_MAX];
    unsigned long long gsz = 0ull;
    { int sl = 0; for (int gi = 0; gi < fg.n; gi++) { slab0[gi] = sl; const int n = split ? fg.nb[gi] : 1; gsz |= (unsigned long long)n << (4 * gi); sl += n; } }
    // one launch of the instantiation K (SweepC<..> / SweepZ<..>) over the group sa holds, on its class's stream
    hipStream_t gs = s;
    const auto launch = [&](auto K) {
        using Kn = decltype(K);
        const int wnb = split ? 1 : sa.nbands;              // bands of a workgroup
        const int nsb = split ? 1 : Kn::nsb(sa.nbands);
        sa.ncb = (nb + 64 * nsb - 1) / (64 * nsb);
        const dim3 sgrid((unsigned)sa.ncb, split ? sa.nbands : 1), sblock(64, wnb * Kn::nt, nsb);
        LAUNCH_LDS(Kn::name.s, Kn::kernel(), sgrid, sblock, Kn::lds_bytes(wnb, nsb), gs, G.D, Wk, sa);
        return 0;
    };
    const auto sweepc = [&](int nq, int phase) {
        if (TUNING && b.idrv == 1) return fail(RRTMG_LW_HIP_EARG, "tuning build: idrv = 0 only");
        return sweepc_dispatch(nq, phase, sweepc_ddt(phase, b.idrv), spec, launch);
    };
    const auto sweepz = [&](int nq) {
        const int zmode = b.mode == 1 ? 1 : b.mode == 3 ? (b.mc ? 3 : 4) : 2;
        if (!sweepz_exists(zmode, false)) return fail(RRTMG_LW_HIP_EARG, "tuning build: rtrnmr only");
        if (!sweepz_exists(zmode, b.idrv == 1)) return fail(RRTMG_LW_HIP_EARG, "tuning build: idrv = 0 only");
        return sweepz_dispatch(nq, zmode, b.idrv == 1, spec, launch);
    };
    for (int phase = 0; phase < 3; phase++) {
        if (b.mode == 0 && phase != 0) continue;                    // (a cloud-free call: phase 0 is all of it)
        if (phase != 1 && one_sweep(nb, b.mode)) continue;          // (the cloud-zone kernel walks all levels of a small batch)
        for (int gi = 0; gi < fg.n; gi++) {                         // one launch per group
            const int nq = fg.gq[gi];
            sa.bands = fg.bands[gi];
            sa.nbands = fg.nb[gi];
            sa.group = slab0[gi];
            gs = (fan && nq < 4) ? SS.q[3 - nq].get() : s;
            int rc = 0;
            if (phase == 1) rc = sweepz(nq);                        // the cloud zone
            else if (b.mode == 0) rc = TUNING ? fail(RRTMG_LW_HIP_EARG, "tuning build: cloudy calls only") : sweepc(nq, 0);
            else if (phase == 0) { rc = sweepc(nq, 1); if (rc == 0 && cfree) rc = sweepc(nq, 0); }      // above the clouds ...
            else rc = sweepc(nq, 2);
            if (rc) return rc;
        }
    }
    if (fan) {
        for (int k = 0; k < 3; k++) {
            HIP_TRY(hipEventRecord(SS.done[k].get(), SS.q[k].get()));
            HIP_TRY(hipStreamWaitEvent(s, SS.done[k].get(), 0));
        }
    }
    {
        // a window of positions x a chunk of levels per workgroup
        const dim3 wgrid((nb + COLSORT_WIN - 1) / COLSORT_WIN, (b.nlay + 1 + FLUX_CH - 1) / FLUX_CH), wblock(COLSORT_WIN);
        const double *pz = GCM ? g.plev : c.pz;
        if (out.uflx_var || out.dflx_var || out.hr_var) {      // the call also wants sample variances: sample 0 zeroes them, sample cnt - 1 updates them
            const double ns = (double)b.nsamp, cnt = b.acc == 0 ? 1.0 : (b.acc == 2 ? ns : (double)b.isamp + 1.0);
            with_const<0, 1, 2, 3, 4, 5>((b.idrv == 1 ? 3 : 0) + b.acc, [&](auto V) {
                constexpr int v = decltype(V)::value;
                LAUNCH("k_flux_var", (k_flux_var<(v >= 3), v % 3>), wgrid, wblock, s, G.D, Wk, out, pz, nb, b.col0, b.nct, b.mode == 0 ? 1 : 0, fg.n, gsz, cfree ? 1 : 0, ns, cnt);
                return 0;
            });
        } else
        if (b.acc != 0) {           // a later sample of an averaging call: its total-sky values join what the caller's arrays hold
            const double ns = (double)b.nsamp;
            with_const<0, 1, 2, 3>((b.idrv == 1 ? 2 : 0) + (b.acc == 2 ? 1 : 0), [&](auto V) {
                constexpr int v = decltype(V)::value;
                LAUNCH("k_flux_acc", (k_flux_acc<(v & 2) != 0, (v & 1) != 0>), wgrid, wblock, s, G.D, Wk, out, pz, nb, b.col0, b.nct, b.mode == 0 ? 1 : 0, fg.n, gsz, cfree ? 1 : 0, ns);
                return 0;
            });
        } else
        if (b.idrv == 1) LAUNCH("k_flux", (k_flux<true>), wgrid, wblock, s, G.D, Wk, out, pz, nb, b.col0, b.nct, b.mode == 0 ? 1 : 0, fg.n, gsz, cfree ? 1 : 0);
        else LAUNCH("k_flux", (k_flux<false>), wgrid, wblock, s, G.D, Wk, out, pz, nb, b.col0, b.nct, b.mode == 0 ? 1 : 0, fg.n, gsz, cfree ? 1 : 0);
    }
    return launches_ok();
}


// one batch on one stream (host-pointer entries, whose staging buffer serialises the batches anyway)
template <bool GCM>
int run_batch(hipStream_t s, const Batch &b, const GcmIn &g, const ColIn &c, const FluxOut &out)
{
    const Workspace Wk = ws_for(0, use_colsort(GCM, b.mode, b.nb) && !b.mc);
    if (int rc = run_prep<GCM>(s, Wk, b, g, c)) return rc;
    if (int rc = run_layer<GCM>(s, Wk, b, g, c)) return rc;
    return run_sweep<GCM>(s, Wk, b, g, c, out);
}

// ---- gas optics (rrtmg_lw_hip_gas_optics*) ------------------------------------------------------------------------------------------
// The optics pipeline of a batch is k_colprep (laytrop, the surface Planck terms) and k_optics.  It needs none of the solver's workspace -
// no cell codes, partial slabs or cloud arrays - only the per-column terms and k_optics' wide-window list, in an allocation of its own.
int ensure_optics_ws(int nlay, int ncolb)
{
    if (G.opt_buf && G.opt_nlay == nlay && G.opt_ncolb >= ncolb) return 0;
    if (int rc = drop(G.opt_buf, "gas-optics workspace")) return rc;
    ncolb = std::max(ncolb, G.opt_nlay == nlay ? G.opt_ncolb : 0);
    const size_t n = (size_t)ncolb, L = (size_t)nlay;
    const size_t b_pc = align_up((size_t)NPERCOL * n * 8, 256), b_lt = align_up(n * 4, 256);
    const size_t b_wide = align_up((2 + ((n + LAYER_BLOCK - 1) / LAYER_BLOCK) * L) * 4, 256);
    if (int rc = grow(G.opt_buf, b_pc + b_lt + b_wide, b_pc + b_lt + b_wide, "gas-optics workspace")) return rc;
    G.opt_percol = G.opt_buf.as<double>();
    G.opt_laytrop = (int *)(G.opt_buf.as<char>() + b_pc);
    G.opt_wide = (int *)(G.opt_buf.as<char>() + b_pc + b_lt);
    HIP_TRY(hipMemset(G.opt_wide, 0, 8));
    G.opt_nlay = nlay;
    G.opt_ncolb = ncolb;
    return 0;
}

// one batch of the gas-optics entries on stream s: columns col0 .. col0 + nb - 1 of arrays nct columns wide (inputs and outputs alike;
// of the Batch it reads these, nlay and idrv: all bands)
template <bool GCM>
int run_optics(hipStream_t s, const Batch &b, const GcmIn &g, const ColIn &c, const OptOut &o)
{
    Workspace W{};
    W.ncolb = G.opt_ncolb; W.pcb = G.opt_ncolb; W.nlay = b.nlay; W.err = G.d_err.as<int>();
    W.percol = G.opt_percol; W.laytrop = G.opt_laytrop;
    W.wide = GCM && HAVE_WIDE && g_wide_window ? G.opt_wide : nullptr;
    LAUNCH("k_colprep", (k_colprep<GCM>), dim3((b.nb + 63) / 64), dim3(64), s, G.D, W, g, c, b.nb, b.col0, b.nct, b.idrv, 1, 0);
    const LayerArgs la = layer_args(b, nullptr);
    const unsigned gx = (b.nb + LAYER_BLOCK - 1) / LAYER_BLOCK;
    if (W.wide) HIP_TRY(hipMemsetAsync(W.wide, 0, sizeof(int), s));
    LAUNCH("k_optics", (k_optics<GCM, 0>), dim3(gx, b.nlay, la.nparts), dim3(LAYER_BLOCK), s, G.D, W, g, c, la, o);
    if constexpr (GCM && HAVE_WIDE) {
        if (W.wide) LAUNCH("k_optics<wide>", (k_optics<true, 1>), dim3(gx * b.nlay, la.nparts), dim3(LAYER_BLOCK), s, G.D, W, g, c, la, o);
    }
    return launches_ok();
}

int check_optics(int idrv, const OptOut &o)
{
    if (!o.taug || !o.fracs) return fail(RRTMG_LW_HIP_EARG, "gas optics: taug and fracs are required");
    if (idrv == 1 && !o.dplankbnd) return fail(RRTMG_LW_HIP_EARG, "gas optics: idrv=1 needs dplankbnd_dt");
    return 0;
}

int ensure_pipeline()
{
    if (G.aux) return 0;
    Event *const ev[] = {&G.ev_in, &G.ev_last, &G.ev_fork, &G.ev_join, &G.ev_ready[0], &G.ev_layer[0], &G.ev_done[0], &G.ev_ready[1], &G.ev_layer[1], &G.ev_done[1]};
    int rc = 0;
    for (Event *e : ev) if (rc == 0) rc = make_event(*e);
    if (rc == 0) rc = make_stream(G.aux, 0, 0);          // (the marker of "made" last; a failure leaves none of them)
    if (rc != 0) for (Event *e : ev) (void)e->reset();
    return rc;
}

// all batches of a device-resident call on the caller's stream `s`, the per-column kernels of batch i+1 overlapping the
// heavy kernels of batch i on the auxiliary stream (two prep sets)
// (The sub-column generator of batch i+1 runs beside k_layer of batch i.  Held back until that k_layer is done, so that it runs beside
// the sweeps instead, it gains nothing - measured per 1e6 McICA columns, profiles/HISTORY.md: beside k_layer the generator takes 19.3 ms
// and k_layer 35.7 (26.7 alone, both VALU-bound), beside the sweeps the generator takes its 12.9 ms and k_sweepc 29.1 instead of 19.9 (a sweep work-group needs most
// of a CU's LDS and waits for the generator's work-groups to leave) - 77.5 vs 77.7 ms a step either way, also with the auxiliary stream
// at the lowest priority.  The generator's 12.9 ms are added work, not hidden work.)
int launch_kiss(hipStream_t s, const Workspace &Wk, int ncol, int col0, int nb, int nlay, int icld, int permuteseed, const SubcolIn &in);
// play, cldfr and alpha of a call whose arrays are d.ld columns wide, once more d.ncol wide in the library's own memory (below, with the
// array-form staging)
int stage_generator_arrays(hipStream_t s, const CallDesc &d, int icld_gen, const double **play, const double **cldfr, const double **alpha);

// A device-resident call of ONE batch that does not fill the chip is a chain of a dozen dependent launches on up to four streams: the
// kernels themselves take two thirds of its time, launch gaps and cross-stream event hops the rest (profiles/round4_small_calls.md).  The
// second call with the same arguments - shape, flags, every array pointer: a host model hands over the same arrays time step after time
// step - is captured (hipStreamBeginCapture on a stream of the library's own) and every later one replays the instantiated graph with one
// hipGraphLaunch on the caller's stream.  rrtmg_lw_hip_set_graph_max / RRTMG_LW_GRAPH_MAX: the largest call (columns) taken this way;
// 0 = never.  Same kernels, same arguments: same results.
int g_graph_max = []() { const char *e = getenv("RRTMG_LW_GRAPH_MAX"); return e ? std::max(0, atoi(e)) : 16384; }();
constexpr size_t GRAPH_CACHE = 8;
void graphs_clear()
{
    G.graphs.clear();
}
template <class T> void key_put(std::vector<unsigned char> &k, const T &v)
{
    const unsigned char *p = reinterpret_cast<const unsigned char *>(&v);
    k.insert(k.end(), p, p + sizeof(T));
}

struct KissGen { bool on; int icld, permuteseed; const double *alpha; };      // kissvec generator folded into the per-batch prep

int run_pipelined(hipStream_t s, const Batch &call, const GcmIn &g, const FluxOut &out, KissGen gen = KissGen{false, 0, 0, nullptr})
{
    if (int rc = ensure_pipeline()) return rc;
    // (ncol: the columns of the call; call.nct, the width of its arrays, only travels to the kernels)
    const int ncol = call.ncall, nlay = call.nlay, mode = call.mode, idrv = call.idrv;
    const McIn *const mc = call.mc;
    const int nbmax = balanced_batch(ncol, eff_batch(nlay));
    // a call that is ONE batch has nothing for its per-column kernels to run beside: they go on the caller's stream, one cross-stream
    // event hop (~20 us of a 0.6 ms call) less
    const bool single = ncol <= nbmax && !(G.split_sweep && G.cu_layer > 0);
    const hipStream_t aux = single ? s : G.aux.get();
    ColIn c{};
    // sub-column arrays mode keeps per-g-point cloud arrays (odg/cfef) in one set only: no layer/sweep overlap there
    const bool split = G.split_sweep && G.ws.two_scr && !(mode == 3 && mc);
    const bool part = split && G.cu_layer > 0;
    if (part && !G.lay_m) {
        if (int rc = make_stream(G.lay_u, 0, 0)) return rc;
        if (int rc = make_stream(G.lay_m, 0, G.cu_layer)) return rc;
    }
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the workspace
    // a small one-batch call as a graph (above): replay, capture (second call with this key), or the plain launches
    State::GraphEnt *gent = nullptr;
    bool capture = false;
    if (single && !split && !gen.on && !mc && !G.profile && !G.n1 && ncol <= g_graph_max) {
        std::vector<unsigned char> key;
        key_put(key, ncol); key_put(key, call.nct); key_put(key, nlay); key_put(key, mode); key_put(key, idrv); key_put(key, call.inflag); key_put(key, call.iceflag); key_put(key, call.liqflag);
        const double *gp[] = {g.play, g.plev, g.tlay, g.tlev, g.tsfc, g.h2ovmr, g.o3vmr, g.co2vmr, g.ch4vmr, g.n2ovmr, g.o2vmr, g.cfc11vmr, g.cfc12vmr,
                              g.cfc22vmr, g.ccl4vmr, g.emis, g.cldfr, g.taucld, g.cicewp, g.cliqwp, g.reice, g.reliq, g.tauaer, g.tauctot,
                              out.uflx, out.dflx, out.hr, out.uflxc, out.dflxc, out.hrc, out.duflx_dt, out.duflxc_dt, out.fnet, out.fnetc,
                              out.uflxs, out.dflxs, out.uflxcs, out.dflxcs, out.uflx_var, out.dflx_var, out.hr_var};
        key_put(key, gp);
        // (what else decides which kernels run with which arguments: the workspace, the tuning switches)
        // (what the kernel nodes carry BY VALUE: the tables of this initialisation - DevTables with heatfac and the table pointers - on its device)
        key_put(key, G.init_gen); key_put(key, G.device);
        key_put(key, G.ws_buf.get()); key_put(key, G.ws_buf.bytes()); key_put(key, g_colsort); key_put(key, g_colsort_min); key_put(key, g_colsort_clear); key_put(key, g_clear_groups); key_put(key, g_one_sweep_max);
        key_put(key, g_wide_window); key_put(key, g_layer_split); key_put(key, g_prep_fork); key_put(key, G.sweep_fanout); key_put(key, eff_batch(nlay)); key_put(key, g_split_max);
        for (auto &e : G.graphs) if (e.key == key) { gent = &e; break; }
        if (!gent) {
            if (G.graphs.size() >= GRAPH_CACHE) {           // the entry used longest ago makes room
                size_t old = 0;
                for (size_t j = 1; j < G.graphs.size(); j++) if (G.graphs[j].used < G.graphs[old].used) old = j;
                G.graphs.erase(G.graphs.begin() + (long)old);
            }
            G.graphs.emplace_back();
            gent = &G.graphs.back();
            gent->key = key;
        }
        gent->used = ++G.graph_clock;
        if (gent->exec) {
            HIP_TRY(hipGraphLaunch(gent->exec.get(), s));
            G.graph_replays++;
            HIP_TRY(hipEventRecord(G.ev_last.get(), s));
            G.ev_last_valid = true;
            return 0;
        }
        // the first call with a key takes the plain launches (whatever is set up lazily - streams, kernel attributes - then exists), the
        // second is captured
        capture = gent->seen >= 1 && !gent->failed;
        gent->seen++;
        if (capture && !G.cap) { if (int rc = make_stream(G.cap, 0, 0)) return rc; }
    }
    const hipStream_t s_call = s;
    if (capture) {
        if (hipStreamBeginCapture(G.cap.get(), hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); capture = false; gent->failed = true; }
        else s = G.cap.get();
    }
    const hipStream_t aux_ = capture ? s : aux;
    if (!single) {
        HIP_TRY(hipEventRecord(G.ev_in.get(), s));             // inputs are ready when the caller's stream gets here
        HIP_TRY(hipStreamWaitEvent(aux, G.ev_in.get(), 0));
    }
    int i = 0, rc_cap = 0;
    Batch b = call;
    // The per-column kernels of batch j on the auxiliary stream, once prep set j & 1 is free again (sweep of batch j-2 done).
    // (They thus run beside k_layer of batch j-1.  Their few long-lived waves cost whatever runs beside
    // them about what the overlap saves - measured per 1e6 columns: k_layer 32.7 ms beside them, 28.3 alone, step 93.9 vs 96.0 on one
    // stream; held back until k_layer is done they slow the sweep instead, 94.4, and the McICA generator then costs 7 ms more.)
    const auto prep = [&](int j) -> int {
        Batch bj = call;
        bj.col0 = j * nbmax; bj.nb = std::min(nbmax, ncol - bj.col0);
        const int kj = j & 1;
        const Workspace Wj = ws_for(kj, use_colsort(true, mode, bj.nb) && !mc);
        if (j >= 2) HIP_TRY(hipStreamWaitEvent(aux, G.ev_done[kj].get(), 0));
        if (int rc = run_prep<true>(aux, Wj, bj, g, c, single && g_prep_fork ? G.aux.get() : nullptr)) return rc;
        if (gen.on) {
            if (int rc = launch_kiss(aux, Wj, call.nct, bj.col0, bj.nb, nlay, gen.icld, gen.permuteseed, SubcolIn{g.play, g.cldfr, gen.alpha})) return rc;
        }
        if (!single) HIP_TRY(hipEventRecord(G.ev_ready[kj].get(), aux));
        return 0;
    };
    // The default pipeline enqueues them BEFORE the sweeps of batch j-1.  A process has fewer hardware queues than this pipeline has
    // streams (the caller's, the auxiliary one, three for the sweeps; four queues by default), so the auxiliary stream shares a queue with
    // a sweep stream, and a queue takes its packets in the order they were enqueued: behind the sweeps of batch j-1, which wait for that
    // batch's k_layer, the per-column kernels ran only when those sweeps were done - beside k_flux, which then took 1.42 ms instead of
    // 0.54 (profiles/flux_walk.md).  (The McICA generator keeps its place: measured where it is.)
    const bool ahead = !single && !split && !capture && !gen.on;
    for (int col0 = 0; col0 < ncol; col0 += nbmax, i++) {
        const int nb = std::min(nbmax, ncol - col0), k = i & 1;
        b.nb = nb; b.col0 = col0;
        const Workspace Wk = ws_for(k, use_colsort(true, mode, nb) && !mc);
        if (capture) {
            // (one batch, one stream: the batch's launches, the fork to the sweep streams and their join become the graph; an error ends
            // the capture before it is reported)
            rc_cap = run_prep<true>(s, Wk, b, g, c, g_prep_fork ? G.aux.get() : nullptr);
            if (rc_cap == 0) rc_cap = run_layer<true>(s, Wk, b, g, c);
            if (rc_cap == 0) rc_cap = run_sweep<true>(s, Wk, b, g, c, out);
            continue;
        }
        if (!ahead || i == 0) { if (int rc = prep(i)) return rc; }
        // (with a CU partition nothing is enqueued on the caller's stream inside the loop: streams with a CU mask are blocking streams, and
        // where the caller's stream is the null stream every operation on it would be a barrier between them)
        if (!part && !single) HIP_TRY(hipStreamWaitEvent(s, G.ev_ready[k].get(), 0));
        if (split) {
            // k_layer of this batch on the caller's stream, its sweep on the sweep set's main stream: the HBM-bound sweep of batch i
            // overlaps the issue-bound k_layer of batch i+1 (scratch set k is free once the sweep of batch i-2 is done).
            // With a CU partition (rrtmg_lw_hip_set_cu_partition) the two run on their own CUs: k_layer's workgroups otherwise take every
            // register and LDS slot of whichever CU they reach first and the sweep workgroups (one per CU: the transmittance table) trickle
            // in behind them.  The first batch's k_layer and the last batch's sweeps have nothing beside them and take the whole chip.
            const bool last = col0 + nbmax >= ncol;
            hipStream_t sl = s;
            int sset = 0;
            if (part) { sl = i == 0 ? G.lay_u.get() : G.lay_m.get(); sset = last ? 0 : 1; }
            if (int rc = ensure_sweep_set(sset)) return rc;
            const hipStream_t ssm = G.swset[sset].main.get();
            if (part) {
                if (i == 0) HIP_TRY(hipStreamWaitEvent(sl, G.ev_in.get(), 0));
                HIP_TRY(hipStreamWaitEvent(sl, G.ev_ready[k].get(), 0));
                if (i >= 1) HIP_TRY(hipStreamWaitEvent(sl, G.ev_layer[(i - 1) & 1].get(), 0));     // (k_layer launches stay in batch order across the two streams)
            }
            if (i >= 2) HIP_TRY(hipStreamWaitEvent(sl, G.ev_done[k].get(), 0));
            if (int rc = run_layer<true>(sl, Wk, b, g, c)) return rc;
            HIP_TRY(hipEventRecord(G.ev_layer[k].get(), sl));
            HIP_TRY(hipStreamWaitEvent(ssm, G.ev_layer[k].get(), 0));
            if (part && i >= 1) HIP_TRY(hipStreamWaitEvent(ssm, G.ev_done[(i - 1) & 1].get(), 0));   // (the partial slabs and the hand-off array exist once: sweeps stay in batch order across the two sets)
            if (int rc = run_sweep<true>(ssm, Wk, b, g, c, out, sset)) return rc;
            HIP_TRY(hipEventRecord(G.ev_done[k].get(), ssm));
        } else {
            if (int rc = run_layer<true>(s, Wk, b, g, c)) return rc;
            if (ahead && col0 + nbmax < ncol) { if (int rc = prep(i + 1)) return rc; }
            if (int rc = run_sweep<true>(s, Wk, b, g, c, out)) return rc;
            HIP_TRY(hipEventRecord(G.ev_done[k].get(), s));
        }
    }
    if (capture) {
        (void)aux_;
        Graph graph;             // (the capture's own graph: gone once it is instantiated, or not)
        const hipError_t ce = hipStreamEndCapture(G.cap.get(), graph.slot());
        s = s_call;
        if (rc_cap != 0) { gent->failed = true; return rc_cap; }
        hipGraphExec_t exec = nullptr;
        if (ce != hipSuccess || !graph || hipGraphInstantiate(&exec, graph.get(), nullptr, nullptr, 0) != hipSuccess) {
            // no graph on this runtime for this call shape: the plain launches, now and from here on
            (void)hipGetLastError();
            graph.reset();
            gent->failed = true;
            return run_pipelined(s, call, g, out, gen);
        }
        graph.reset();
        *gent->exec.slot() = exec;
        G.graph_captures++;
        HIP_TRY(hipGraphLaunch(gent->exec.get(), s));
    }
    if (split) {                                  // the caller's stream sees the results of every batch
        for (int k = 0; k < std::min(i, 2); k++) HIP_TRY(hipStreamWaitEvent(s, G.ev_done[k].get(), 0));
    }
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return 0;
}

// All batches of a device-resident call that averages nsamp sub-column samples, on the caller's stream: batch by batch, and within a
// batch sample by sample, so that what the samples of a batch share stays where it is - the gas codes, the binary-key words and the
// float64 optical depths that k_layer leaves with the first sample (Batch::share).  Per sample: the per-column kernels, the generator
// with that sample's seed, k_cloudmc<mask> and k_blocksort, k_layer (sample 0) or k_codet (the others), the sweeps, k_flux (Batch::acc).
// One prep set, one scratch set, no auxiliary stream: a sample's kernels depend on each other, and the next sample's mask, cloud flags
// and hand-off levels go where this one's are.
int run_samples(hipStream_t s, const Batch &call, const GcmIn &g, const FluxOut &out, KissGen gen, int nsamp, int seedstep)
{
    if (int rc = ensure_pipeline()) return rc;
    const int ncol = call.ncall, nlay = call.nlay;
    const int nbmax = balanced_batch(ncol, eff_batch(nlay));
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the workspace
    ColIn c{};
    Batch b = call;
    b.nsamp = nsamp;
    for (int col0 = 0; col0 < ncol; col0 += nbmax) {
        b.nb = std::min(nbmax, ncol - col0); b.col0 = col0;
        const Workspace Wk = ws_for(0, use_colsort(true, call.mode, b.nb));
        for (int i = 0; i < nsamp; i++) {
            b.acc = i == 0 ? 0 : (i == nsamp - 1 ? 2 : 1);
            b.share = i == 0 ? 1 : 2;
            b.isamp = i;
            const int seed = (int)((long long)gen.permuteseed + (long long)i * seedstep);
            if (int rc = run_prep<true>(s, Wk, b, g, c)) return rc;
            if (int rc = launch_kiss(s, Wk, call.nct, b.col0, b.nb, nlay, gen.icld, seed, SubcolIn{g.play, g.cldfr, gen.alpha})) return rc;
            if (int rc = run_layer<true>(s, Wk, b, g, c)) return rc;
            if (int rc = run_sweep<true>(s, Wk, b, g, c, out)) return rc;
        }
    }
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return 0;
}

int read_physics_error(hipStream_t s)
{
    int code = 0;
    HIP_TRY(hipMemcpyAsync(&code, G.d_err.as<int>(), sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (code != 0) {
        int zero = 0;
        HIP_TRY(hipMemcpy(G.d_err.as<int>(), &zero, sizeof(int), hipMemcpyHostToDevice));
        return fail(RRTMG_LW_HIP_EPHYSICS, "%s", physics_message(code));
    }
    return 0;
}

int ensure_stage(size_t bytes)
{
    return grow(G.stage_buf, bytes, bytes, "host-entry staging");
}

// the McICA entries exist in both builds: ngptlw sub-columns (src/rrtmg_lw_rad.f90:140, :267-288), masks of MASK_WORDS words
int check_mcica_build()
{
    return 0;
}

int check_common(int ncol, int nlay)
{
    if (!G.init) return fail(RRTMG_LW_HIP_ENOTINIT, "rrtmg_lw_hip_init has not been called");
    if (ncol < 1 || nlay < 1 || nlay > 603) return fail(RRTMG_LW_HIP_EARG, "bad dimensions ncol=%d nlay=%d", ncol, nlay);
    return 0;
}

// Spectral outputs of the *_spectral entries: per band the flux the band adds to the broadband one (ncol,nlay+1,16), uflxs and dflxs
// required, the clear-sky pair both null or both set.  They reach the sweeps through FluxOut (run_sweep: the SPEC instantiations).
int check_spec(const FluxOut &o)
{
    if (!o.uflxs || !o.dflxs) return fail(RRTMG_LW_HIP_EARG, "spectral entry: uflxs and dflxs are required");
    if (!o.uflxcs != !o.dflxcs) return fail(RRTMG_LW_HIP_EARG, "spectral entry: uflxcs and dflxcs must be both null or both set");
    return 0;
}
// what the rrtmg_lw entries check first; an icld out of range comes back as 2 (src/rrtmg_lw_rad.nomcica.f90:456, src/rrtmg_lw_rad.f90:469)
int check_call(const CallDesc &d, const FluxOut &out)
{
    if (int rc = check_common(d.ncol, d.nlay)) return rc;
    if (d.spectral) if (int rc = check_spec(out)) return rc;
    if (!d.icld) return fail(RRTMG_LW_HIP_EARG, "icld is null");
    if (*d.icld < 0 || *d.icld > 3) *d.icld = 2;
    if (d.idrv == 1 && (!out.duflx_dt || !out.duflxc_dt)) return fail(RRTMG_LW_HIP_EARG, "idrv=1 needs duflx_dt and duflxc_dt");
    return 0;
}

// ---- host-pointer staging ---------------------------------------------------------------------------
// Every array of the interface is [rows][ncol][inner] with `inner` fastest (inner = 1 for (ncol,nlay) arrays,
// 16 for taucld, 140 for the McICA sub-column arrays); a column block is therefore one 2-D copy.
// The pipelined entries (host_pipeline) fill `src` per batch: where the batch's rows are read from - the caller's array, or an entry's
// own pinned scratch for an array it reduces on the host (tauctot).
struct HostIn {
    const double *h; size_t inner, rows; double *d;
    bool pinned = false;                                  // h is page-locked (rrtmg_lw_hip_host_register, or pinned by the caller's own means)
    const double *src = nullptr; size_t src_ncol = 0, src_col0 = 0; bool src_pinned = false;
    const unsigned char *skip = nullptr;                  // per batch, set by the entry's prep step: rows nothing reads (a cloud array's layers without cloud) - not scanned, zero-filled
    const unsigned char *known = nullptr;                 // ... rows the prep step has already read in full and found to hold one pattern (known_bits): not scanned again
    const uint64_t *known_bits = nullptr;
    unsigned long long static_gen = 0;                    // != 0: the caller declared the array static (rrtmg_lw_hip_host_static): row scans are cached per batch
    // bytes per element of h (4: a *_r4 entry's float array behind the double pointer) and of the batch's src (8 again where the entry
    // names its own float64 scratch, tauctot); land: the array's rows in the staging set's float32 landing area, where 4-byte rows arrive
    size_t esz = 8, src_esz = 8;
    float *land = nullptr;
};
struct HostOut { double *h; size_t rows; double *d; bool active; bool pinned = false; size_t esz = 8; float *land = nullptr; };
using hostrows::land_stride;
using hostrows::widened_bits;
// Where input `a` stands in a call's staged list: tauaer before the cloud arrays (the order of the rows in the device buffer and of the copies)
constexpr int staged_at(int a) { return a < A_CLDFR ? a : a == A_TAUAER ? (int)A_CLDFR : a + 1; }

// The staged inputs of a host-pointer call, the first n of rrtmg_lw's arrays (gas optics: the 16 up to emis), and their null checks.
// The cloud arrays travel only with `cloud` - the McICA entry's sub-column arrays `m` in their places - and taucld with tau_inner values
// per (column, layer).
int host_ins(std::vector<HostIn> &ins, const GcmIn &g, const McIn *m, size_t L, bool cloud, size_t tau_inner, int n = NA_GCM, const char *who = "", size_t esz = 8)
{
    const double *p[NA_IN];
    gcm_pointers(g, nullptr, p);
    if (m) { p[A_CLDFR] = m->cldfmcl; p[A_TAUCLD] = m->taucmcl; p[A_CICEWP] = m->ciwpmcl; p[A_CLIQWP] = m->clwpmcl; p[A_REICE] = m->reicmcl; p[A_RELIQ] = m->relqmcl; }
    ins.assign((size_t)n, HostIn{});
    for (int a = 0; a < n; a++) {
        // (McICA: cldfmcl, taucmcl, ciwpmcl, clwpmcl are (ngpt,ncol,nlay); reicmcl and relqmcl (ncol,nlay) like reice and reliq)
        const size_t inner = m && a >= A_CLDFR && a <= A_CLIQWP ? (size_t)NGPT : a == A_TAUCLD ? tau_inner : CALL_ARRAYS[a].inner;
        ins[staged_at(a)] = HostIn{CALL_ARRAYS[a].cloud && !cloud ? nullptr : p[a], inner, rows_of(a, L), nullptr};
        ins[staged_at(a)].esz = esz;
    }
    for (int a = 0; a < n; a++) if (!CALL_ARRAYS[a].cloud && !p[a]) return fail(RRTMG_LW_HIP_EARG, "%snull input array (argument %d)", who, a);
    for (int a = 0; a < n; a++) if (cloud && CALL_ARRAYS[a].cloud && !p[a]) return fail(RRTMG_LW_HIP_EARG, m ? "null McICA cloud array" : "null cloud array");
    return 0;
}
// ... and a batch's staged device arrays as run_batch takes them
GcmIn staged_gcm(const std::vector<HostIn> &in)
{
    const double *p[NA_IN] = {};
    for (int a = 0; a < (int)in.size(); a++) p[a] = in[staged_at(a)].d;
    return gcm_from(p);
}
// a batch's layers without cloud, found by rows_below on the cloud fraction: those rows of it have just been read to their end, the
// other cloud arrays are not read there (nor summed, nor scanned, nor copied)
void skip_cloudfree(std::vector<HostIn> &ins, const unsigned char *cloudfree, const unsigned char *uniform, const uint64_t *bits)
{
    ins[staged_at(A_CLDFR)].known = uniform; ins[staged_at(A_CLDFR)].known_bits = bits;
    for (int a = A_TAUCLD; a <= A_RELIQ; a++) ins[staged_at(a)].skip = cloudfree;
}
// The staged outputs: the eight broadband arrays (the derivatives active with idrv = 1), then the spectral four (no rows when absent)
std::vector<HostOut> host_outs(const FluxOut &o, size_t L, int idrv, size_t esz = 8)
{
    double *p[NA_CALL];
    flux_pointers(o, p);
    std::vector<HostOut> outs;
    for (int a = A_UFLX; a < A_UFLXS; a++) outs.push_back({p[a], rows_of(a, L), nullptr, a < A_DUFLX_DT || idrv == 1});
    for (int a = A_UFLXS; a < NA_CALL; a++) outs.push_back({p[a], p[a] ? rows_of(a, L) : 0, nullptr, p[a] != nullptr});
    for (auto &a : outs) a.esz = esz;
    return outs;
}
FluxOut staged_flux(const std::vector<HostOut> &v)
{
    double *p[NA_CALL];
    for (int a = A_UFLX; a < NA_CALL; a++) p[a] = a < A_UFLXS || v[a - A_UFLX].active ? v[a - A_UFLX].d : nullptr;
    return flux_from(p);
}
int bounce_h2d(void *dst, const void *src, size_t bytes);
int bounce_d2h(void *dst, const void *src, size_t bytes);
int bounce_h2d_rows(void *dst, const void *src, size_t row_bytes, size_t stride_bytes, size_t rows);

int stage_alloc(std::vector<HostIn> &ins, std::vector<HostOut> &outs, size_t nb)
{
    size_t tot = 0;
    for (auto &a : ins) tot += a.h ? a.inner * a.rows * nb : 0;
    for (auto &a : outs) tot += a.rows * nb;
    if (int rc = ensure_stage(tot * 8 + 4096)) return rc;
    double *p = G.stage_buf.as<double>();
    for (auto &a : ins) { a.d = a.h ? p : nullptr; p += a.h ? a.inner * a.rows * nb : 0; }
    for (auto &a : outs) { a.d = p; p += a.rows * nb; }
    return 0;
}

// the plain form (small one-batch entries: get_alpha, the stand-alone generator): blocking copies through the library's pinned buffer (bounce_h2d)
int stage_in(std::vector<HostIn> &ins, size_t ncol, size_t col0, size_t nb, hipStream_t s)
{
    HIP_TRY(hipStreamSynchronize(s));                    // (the staging buffer's last readers)
    for (auto &a : ins) {
        if (!a.h) continue;
        const size_t w = a.inner * nb * 8;
        if (nb == ncol) { if (int rc = bounce_h2d(a.d, a.h, w * a.rows)) return rc; continue; }
        if (int rc = bounce_h2d_rows(a.d, a.h + a.inner * col0, w, a.inner * ncol * 8, a.rows)) return rc;
    }
    return 0;
}

int stage_out(std::vector<HostOut> &outs, size_t ncol, size_t col0, size_t nb, hipStream_t s)
{
    HIP_TRY(hipStreamSynchronize(s));
    for (auto &a : outs) {
        if (!a.active || !a.h) continue;
        const size_t w = nb * 8;
        if (nb == ncol) { if (int rc = bounce_d2h(a.h, a.d, w * a.rows)) return rc; continue; }
        for (size_t r = 0; r < a.rows; r++)
            if (int rc = bounce_d2h(a.h + col0 + ncol * r, a.d + nb * r, w)) return rc;
    }
    return 0;
}

// f(t, nt) on nt host threads (the host-pointer entries' own work on the caller's arrays: row scans, packing, tauctot)
int host_threads()
{
    static const int nt = []() {         // (initialised once, thread-safe: the fan-out's worker threads all come through here)
        const char *e = getenv("RRTMG_LW_HOST_THREADS");
        int v = e ? atoi(e) : (int)std::thread::hardware_concurrency();
#ifdef __linux__
        cpu_set_t set;
        if (!e && sched_getaffinity(0, sizeof set, &set) == 0) v = std::min(v, CPU_COUNT(&set));
#endif
        return std::max(1, std::min(v, e ? 64 : 16));     // (sixteen unless the variable asks for more: the scan is bound by the memory of the NUMA node the arrays live on)
    }();
    return nt;
}
// The host threads persist (a batch of the host-pointer entries has three parallel regions of a millisecond or two each: fifteen thread
// starts per region cost a fifth of that).  One region at a time: a second caller - the worker thread of another device of the fan-out -
// starts its own threads instead of waiting.
class HostPool {
    std::mutex use_, mu_;
    std::condition_variable go_, done_;
    std::vector<std::thread> th_;
    const std::function<void(int, int)> *job_ = nullptr;
    int nt_ = 0, pending_ = 0;
    unsigned long long gen_ = 0;
    bool stop_ = false;
    void worker(int t)
    {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int, int)> *job;
            int nt;
            {
                std::unique_lock<std::mutex> lk(mu_);
                go_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_; job = job_; nt = nt_;
            }
            if (t < nt) {
                (*job)(t, nt);
                std::lock_guard<std::mutex> lk(mu_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
public:
    ~HostPool()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        go_.notify_all();
        for (auto &x : th_) x.join();
    }
    // f(t, nt) for t = 0 .. nt - 1 (t = 0 on the calling thread); false when the pool is in use
    bool run(int nt, const std::function<void(int, int)> &f)
    {
        std::unique_lock<std::mutex> use(use_, std::try_to_lock);
        if (!use.owns_lock()) return false;
        while ((int)th_.size() < nt - 1) { const int t = (int)th_.size() + 1; th_.emplace_back([this, t] { worker(t); }); }
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f; nt_ = nt; pending_ = nt - 1; gen_++;
        }
        go_.notify_all();
        f(0, nt);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
        return true;
    }
};
// One pool per device of the fan-out: the worker thread that feeds device d (fan_out) runs its parallel regions on pool d with its share
// of the host threads (host_threads() / devices: the scans are bound by the host's memory, more threads than cores only take turns).
HostPool g_pools[MAXDEV];
thread_local int tl_pool = 0, tl_share = 1;

template <class F>
void host_parallel(size_t work_bytes, F f)
{
    // (a thread per MB of host data at least: a call of a few columns does not wake sixteen threads)
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, host_threads() / tl_share), work_bytes >> 20));
    if (nt == 1) { f(0, 1); return; }
    const std::function<void(int, int)> fn = [&f](int t, int n) { f(t, n); };
    if (g_pools[tl_pool].run(nt, fn)) return;
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back([=, &f]() { f(t, nt); });
    f(0, nt);
    for (auto &x : th) x.join();
}

// flags[r] = 1 when every value of row r of the column batch [col0, col0 + nb) of a (rows, ncol, inner) array is below `thr` (a NaN is not).
// With thr = cldmin: a layer of the cloud fraction without cloud in any column of the batch - cldprop / cldprmc then read nothing else of that
// layer (src/rrtmg_lw_cldprop.f90:185-186, src/rrtmg_lw_cldprmc.f90:182-183), so the other cloud arrays' rows of that layer need not be read here.
// uni / bits (optional): rows that were read to their end (the ones below the threshold) and hold ONE 8-byte pattern - stage_rows need not read them again.
// T = float (the *_r4 entries): 4-byte patterns, compared with the widened threshold as the widened values would be; bits: the widened value's.
template <class T>
void rows_below(const T *h, size_t inner, size_t rows, size_t ncol, size_t col0, size_t nb, double thr, unsigned char *flags,
                unsigned char *uni = nullptr, uint64_t *bits = nullptr)
{
    using U = hostrows::Pattern<T>;
    host_parallel(inner * rows * nb * sizeof(T), [&](int t, int nt) {
        for (size_t r = (size_t)t; r < rows; r += (size_t)nt) {
            const T *p = h + inner * (col0 + ncol * r);
            const U *u = reinterpret_cast<const U *>(p);
            const size_t n = inner * nb;
            const U v = u[0];
            U acc = 0;
            bool below = true;
            size_t i = 0;
            for (; i + 64 <= n && below; i += 64) {
                int ok = 1;
                for (size_t e = 0; e < 64; e++) { ok &= (int)(p[i + e] < thr); acc |= u[i + e] ^ v; }
                below = ok != 0;
            }
            for (; i < n && below; i++) { below = p[i] < thr; acc |= u[i] ^ v; }
            flags[r] = below ? 1 : 0;
            if (uni) { uni[r] = (below && acc == 0) ? 1 : 0; bits[r] = widened_bits(p[0]); }
        }
    });
}

// Ranges pinned through rrtmg_lw_hip_host_register (and the chunk queue's own pinned set): an array lies in one of them with all its bytes,
// or it is treated as pageable and goes through the pinned staging.  (The runtime's pointer attributes were asked as well, at an array's
// first and last byte, until tools/soak_host_entry.py found the hole: registrations are page-granular, so an UNREGISTERED array whose two
// ends share pages with registered neighbours - small arrays side by side on the heap - looked pinned, its middle pages were not mapped for
// the device, and the direct copy faulted.  An array pinned by other means than this library's call is copied like a pageable one.)
std::vector<std::pair<const char *, size_t>> g_pinned;
void forget_pinned(const void *ptr)
{
    for (size_t i = 0; i < g_pinned.size(); i++)
        if (g_pinned[i].first == (const char *)ptr) { g_pinned.erase(g_pinned.begin() + (long)i); break; }
}
bool host_range_pinned(const void *p, size_t bytes)
{
    const char *a = (const char *)p;
    if (!a || bytes == 0) return false;
    for (auto &r : g_pinned)
        if (a >= r.first && a + bytes <= r.first + r.second) return true;
    return false;
}

// Arrays the caller has declared static (rrtmg_lw_hip_host_static): their contents stay as they are until rrtmg_lw_hip_host_changed.
// The host-pointer entries scan every input row of every call for "one value for all columns of the batch" (stage_rows) - 14 KB per
// 72-layer column of reads that bound the entry once the arrays are pinned; for a static array (well-mixed gases handed over as full
// arrays, zero aerosol, emissivities) the answer of the first call is kept per (array, column batch) and the rows are not read again:
// uniform rows are filled on the device as before, the others go straight to their DMA.
struct StaticRange { const char *p; size_t bytes; unsigned long long gen; };
std::vector<StaticRange> g_static;
unsigned long long g_static_gen = 1;
struct ScanKey {
    const void *base; size_t ncol, inner, rows, col0, nb, esz;          // esz: an address seen again with another element type is another array
    bool operator<(const ScanKey &o) const
    {
        if (base != o.base) return base < o.base;
        if (esz != o.esz) return esz < o.esz;
        if (ncol != o.ncol) return ncol < o.ncol;
        if (inner != o.inner) return inner < o.inner;
        if (rows != o.rows) return rows < o.rows;
        if (col0 != o.col0) return col0 < o.col0;
        return nb < o.nb;
    }
};
struct ScanVal { unsigned long long gen = 0; std::vector<unsigned char> state; std::vector<uint64_t> bits; };     // state: 0 not scanned, 1 uniform, 2 not uniform
std::map<ScanKey, ScanVal> g_scan;
std::mutex g_scan_mu;          // (the fan-out's worker threads stage their batches side by side)
// generation of the static range that holds the whole array, 0 if none
unsigned long long static_gen_of(const void *p, size_t bytes)
{
    const char *a = (const char *)p;
    for (auto &r : g_static)
        if (a >= r.p && a + bytes <= r.p + r.bytes) return r.gen;
    return 0;
}

int ensure_hostbuf(PinnedBuf &b, size_t bytes) { return grow(b, bytes, bytes + bytes / 4 + 4096, "pinned host staging"); }

// Blocking copies between the caller's (possibly pageable) memory and the device through this library's own pinned buffer: the runtime is
// never handed a pageable user pointer.  It would pin the range in place, page-granular, and unpin it afterwards - and the unpinning takes a
// page shared with a neighbouring array out of the device's page table as well, whether that neighbour is the source of another copy in
// flight or an array the caller registered (tools/soak_host_entry.py: "Memory access fault" at heap addresses).
constexpr size_t BOUNCE_BYTES = (size_t)32 << 20;
int bounce_h2d(void *dst, const void *src, size_t bytes)
{
    auto &hs = G.hset[0];
    if (int rc = ensure_hostbuf(hs.in, std::min(bytes, BOUNCE_BYTES))) return rc;
    for (size_t o = 0; o < bytes; o += BOUNCE_BYTES) {
        const size_t n = std::min(BOUNCE_BYTES, bytes - o);
        host_parallel(2 * n, [&](int t, int nt) {
            const size_t a = n * (size_t)t / (size_t)nt, b = n * (size_t)(t + 1) / (size_t)nt;
            memcpy(hs.in.as<char>() + a, (const char *)src + o + a, b - a);
        });
        HIP_TRY(hipMemcpy((char *)dst + o, hs.in.get(), n, hipMemcpyHostToDevice));
    }
    return 0;
}
int bounce_d2h(void *dst, const void *src, size_t bytes)
{
    auto &hs = G.hset[0];
    if (int rc = ensure_hostbuf(hs.out, std::min(bytes, BOUNCE_BYTES))) return rc;
    for (size_t o = 0; o < bytes; o += BOUNCE_BYTES) {
        const size_t n = std::min(BOUNCE_BYTES, bytes - o);
        HIP_TRY(hipMemcpy(hs.out.get(), (const char *)src + o, n, hipMemcpyDeviceToHost));
        host_parallel(2 * n, [&](int t, int nt) {
            const size_t a = n * (size_t)t / (size_t)nt, b = n * (size_t)(t + 1) / (size_t)nt;
            memcpy((char *)dst + o + a, hs.out.as<char>() + a, b - a);
        });
    }
    return 0;
}

// `rows` rows of `row_bytes` each, `stride_bytes` apart in the caller's memory, to a contiguous device buffer (a column block of a
// (ncol, nlay) array), packed into the pinned buffer by the host threads first
int bounce_h2d_rows(void *dst, const void *src, size_t row_bytes, size_t stride_bytes, size_t rows)
{
    if (row_bytes == stride_bytes) return bounce_h2d(dst, src, row_bytes * rows);
    auto &hs = G.hset[0];
    const size_t per = std::max<size_t>(1, BOUNCE_BYTES / row_bytes);
    if (int rc = ensure_hostbuf(hs.in, std::min(rows, per) * row_bytes)) return rc;
    for (size_t r0 = 0; r0 < rows; r0 += per) {
        const size_t nr = std::min(per, rows - r0);
        host_parallel(2 * nr * row_bytes, [&](int t, int nt) {
            for (size_t r = nr * (size_t)t / (size_t)nt; r < nr * (size_t)(t + 1) / (size_t)nt; r++)
                memcpy(hs.in.as<char>() + r * row_bytes, (const char *)src + (r0 + r) * stride_bytes, row_bytes);
        });
        HIP_TRY(hipMemcpy((char *)dst + r0 * row_bytes, hs.in.get(), nr * row_bytes, hipMemcpyHostToDevice));
    }
    return 0;
}

int ensure_copy_streams()
{
    if (G.cp_in) return 0;
    int rc = 0;
    for (int k = 0; k < HOST_SETS && rc == 0; k++)
        if ((rc = make_event(G.ev_h2d[k])) == 0 && (rc = make_event(G.ev_cmp[k])) == 0) rc = make_event(G.ev_d2h[k]);
    if (rc == 0 && (rc = make_stream(G.cp_out, 0, 0)) == 0) rc = make_stream(G.cp_in, 0, 0);      // (the marker of "made" last)
    if (rc != 0) {
        G.cp_out.reset();
        for (int k = 0; k < HOST_SETS; k++) { G.ev_h2d[k].reset(); G.ev_cmp[k].reset(); G.ev_d2h[k].reset(); }
    }
    return rc;
}

// One column batch of the input arrays -> device staging (stream s), moving only what has to move:
//  * a row (one layer, or one (layer, band) of tauaer) whose nb x inner values all hold the same 8-byte pattern does not travel: runs of
//    such rows become entries of the k_fill_rows table.  Well-mixed gases handed over as constants, cloud arrays outside the cloudy
//    layers and aerosol optical depths outside the aerosol layers are most of a GCM call's bytes; the device arrays are bit-identical
//    to copied ones.  A row that is not uniform leaves the scan at its first 64 values.
//  * rows of a PAGEABLE array are packed into the pinned set by the host threads and leave as one asynchronous DMA per run of rows
//    (the runtime's own pageable path is one blocking, single-threaded staging copy per call); rows of a pinned array leave from
//    where they lie.
//  * rows of 4-byte values (src_esz = 4, the *_r4 entries) are scanned as 4-byte patterns - the fill writes the widened value -, travel
//    as they are into the staging set's float32 landing area (HostIn::land), every row on a 16-byte boundary there and in the pinned set,
//    and are widened into the float64 array by ONE k_widen_rows launch behind the DMAs (its table: pinned set k, one entry per row).
// The pinned set k is free: the caller has waited for the DMAs of the batch that used it last.
struct StagedRow { unsigned arr, row; bool uniform; uint64_t bits; size_t off; };
// workgroups per table entry of k_widen_rows / k_narrow_rows for rows of up to w values
unsigned cvt_blocks(size_t w) { return (unsigned)std::min<size_t>(CVT_BLOCKS, std::max<size_t>(1, (w + 256 * CVT_LANE - 1) / (256 * CVT_LANE))); }
int stage_rows(std::vector<HostIn> &ins, size_t nb, int k, hipStream_t s)
{
    static thread_local std::vector<StagedRow> tl_rows;
    std::vector<StagedRow> &rows = tl_rows;          // (the host threads below must see THIS thread's list)
    rows.clear();
    size_t bytes = 0, nrows = 0;
    for (auto &a : ins) nrows += a.h ? a.rows : 0;
    rows.reserve(nrows);
    for (size_t ai = 0; ai < ins.size(); ai++) {
        const HostIn &a = ins[ai];
        if (!a.h) continue;
        for (size_t r = 0; r < a.rows; r++) rows.push_back({(unsigned)ai, (unsigned)r, false, 0, 0});
        bytes += a.inner * a.rows * nb * a.src_esz;
    }
    auto row_src = [&](const StagedRow &q) { const HostIn &a = ins[q.arr]; return (const char *)a.src + a.src_esz * a.inner * (a.src_col0 + a.src_ncol * q.row); };
    // cached scans of the arrays declared static (the entry of this array and batch; filled below on a miss)
    std::vector<ScanVal *> cache(ins.size(), nullptr);
    std::vector<unsigned char> cache_hit(ins.size(), 0);
    {
        std::lock_guard<std::mutex> lk(g_scan_mu);
        for (size_t ai = 0; ai < ins.size(); ai++) {
            const HostIn &a = ins[ai];
            if (!a.h || a.static_gen == 0 || a.src != a.h) continue;          // (an array the entry reduces on the host, tauctot, is formed anew per call)
            ScanVal &v = g_scan[ScanKey{a.h, a.src_ncol, a.inner, a.rows, a.src_col0, nb, a.esz}];
            if (v.gen == a.static_gen && v.state.size() == a.rows) cache_hit[ai] = 1;
            else { v.gen = a.static_gen; v.state.assign(a.rows, 0); v.bits.assign(a.rows, 0); }
            cache[ai] = &v;                                                     // (map nodes do not move; entries are dropped under the entry lock only)
        }
    }
    host_parallel(bytes, [&](int t, int nt) {
        for (size_t j = (size_t)t; j < rows.size(); j += (size_t)nt) {
            StagedRow &q = rows[j];
            if (ins[q.arr].skip && ins[q.arr].skip[q.row]) { q.uniform = true; q.bits = 0; continue; }
            if (ins[q.arr].known && ins[q.arr].known[q.row]) { q.uniform = true; q.bits = ins[q.arr].known_bits[q.row]; continue; }
            if (cache_hit[q.arr] && cache[q.arr]->state[q.row] != 0) { q.uniform = cache[q.arr]->state[q.row] == 1; q.bits = cache[q.arr]->bits[q.row]; continue; }
            const size_t n = ins[q.arr].inner * nb;
            // (a float row is uniform when its 4-byte patterns are equal; q.bits: the widened value's, what the fill writes)
            if (ins[q.arr].src_esz == 4) q.uniform = hostrows::row_uniform(reinterpret_cast<const float *>(row_src(q)), n, &q.bits);
            else q.uniform = hostrows::row_uniform(reinterpret_cast<const double *>(row_src(q)), n, &q.bits);
            if (cache[q.arr]) { cache[q.arr]->bits[q.row] = q.bits; cache[q.arr]->state[q.row] = q.uniform ? 1 : 2; }      // (one thread per row)
        }
    });
    size_t need = 0;
    size_t nwiden = 0;
    for (auto &q : rows) {
        const HostIn &a = ins[q.arr];
        if (q.uniform) continue;
        if (a.src_esz == 4) nwiden++;
        if (a.src_pinned) continue;
        if (a.src_esz == 4) { need = align_up(need, 16); q.off = need; need += land_stride(a.inner * nb); }       // (as the row lies in the landing area)
        else { q.off = need; need += a.inner * nb * 8; }
    }
    auto &hs = G.hset[k];
    if (int rc = ensure_hostbuf(hs.in, need)) return rc;
    if (need)
        host_parallel(2 * need, [&](int t, int nt) {
            for (size_t j = (size_t)t; j < rows.size(); j += (size_t)nt) {
                const StagedRow &q = rows[j];
                if (!q.uniform && !ins[q.arr].src_pinned) memcpy(hs.in.as<char>() + q.off, row_src(q), ins[q.arr].inner * nb * ins[q.arr].src_esz);
            }
        });
    RowFill *tab = hs.fill.as<RowFill>();
    if (int rc = ensure_hostbuf(hs.widen, nwiden * sizeof(RowCvt))) return rc;          // (the pipeline has sized it for every row)
    RowCvt *wtab = hs.widen.as<RowCvt>();
    size_t nf = 0, nw = 0, wmax = 0;
    for (size_t j = 0; j < rows.size();) {
        const StagedRow &q = rows[j];
        const HostIn &a = ins[q.arr];
        const size_t w = a.inner * nb;                    // values per row
        size_t j1 = j + 1;
        while (j1 < rows.size() && rows[j1].arr == q.arr && rows[j1].uniform == q.uniform && (!q.uniform || rows[j1].bits == q.bits)) j1++;
        const size_t nr = j1 - j;
        double *dst = a.d + w * q.row;
        if (q.uniform) {
            for (size_t done = 0; done < nr * w; done += FILL_MAX)
                tab[nf++] = RowFill{reinterpret_cast<unsigned long long *>(dst + done), std::min<unsigned long long>(FILL_MAX, nr * w - done), q.bits};
        } else if (a.src_esz == 4) {
            // float32 rows travel as they are into the landing area (a pinned array's from where they lie, 4-byte widths; a pageable
            // array's from the pinned set, packed at the landing area's row stride) and are widened there, one table entry per row
            const size_t st = land_stride(w);
            float *land = a.land + st / 4 * q.row;
            if (a.src_pinned) HIP_TRY(hipMemcpy2DAsync(land, st, row_src(q), a.inner * a.src_ncol * 4, w * 4, nr, hipMemcpyHostToDevice, s));
            else HIP_TRY(hipMemcpyAsync(land, hs.in.as<char>() + q.off, nr * st, hipMemcpyHostToDevice, s));
            for (size_t r = 0; r < nr; r++) wtab[nw++] = RowCvt{dst + w * r, land + st / 4 * r, w};
            wmax = std::max(wmax, w);
        } else if (a.src_pinned) {
            HIP_TRY(hipMemcpy2DAsync(dst, w * 8, row_src(q), a.inner * a.src_ncol * 8, w * 8, nr, hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync(dst, hs.in.as<char>() + q.off, nr * w * 8, hipMemcpyHostToDevice, s));
        }
        j = j1;
    }
    for (size_t f0 = 0; f0 < nf; f0 += 65535)
        hipLaunchKernelGGL(k_fill_rows, dim3(FILL_BLOCKS, (unsigned)std::min<size_t>(65535, nf - f0)), dim3(256), 0, s, (const RowFill *)(tab + f0));
    for (size_t f0 = 0; f0 < nw; f0 += 65535)
        LAUNCH("k_widen_rows", k_widen_rows, dim3(cvt_blocks(wmax), (unsigned)std::min<size_t>(65535, nw - f0)), dim3(256), s, (const RowCvt *)(wtab + f0));
    return 0;
}

// Host-pointer entries as a three-stage pipeline over the column batches: H2D of batch i+1 (copy stream) | kernels of
// batch i (G.stream) | D2H of batch i-1 (second copy stream), HOST_SETS staging sets on the device and as many pinned sets on the host.
// The calling thread (with the host threads) scans and packs batch i+1 and unpacks the outputs of batch i-1 while the DMAs and
// kernels of the batches between are in flight; nothing it calls blocks on a copy.  body(stream, nb, col0, in, out) enqueues the
// kernels of one batch whose staged arrays start at column 0; prep(k, col0, nb, stream) is the entry's own host work for the batch.
// RRTMG_LW_STAGE_TIMING=1: per call, the pipeline prints where its time went (host phases by the clock, device stages by events)
const bool g_stage_timing = []() { const char *e = getenv("RRTMG_LW_STAGE_TIMING"); return e && atoi(e) != 0; }();
struct StageClock {
    double t[8] = {};          // 0 wait h2d, 1 unpack (incl. wait for the D2H), 2 prep, 3 scan + pack + enqueue, 4 body enqueue, 5 copy_out enqueue, 6 final drain
    std::chrono::steady_clock::time_point last;
    void start() { last = std::chrono::steady_clock::now(); }
    void lap(int k) { auto n = std::chrono::steady_clock::now(); t[k] += std::chrono::duration<double, std::milli>(n - last).count(); last = n; }
};
struct NoPrep { int operator()(int, int, int, hipStream_t) const { return 0; } };
template <class Body, class Prep>
int host_pipeline_run(int ncol, int c0, int c1, int nbmax, std::vector<HostIn> &ins, std::vector<HostOut> &outs, Body body, Prep prep, std::vector<Event> &tev);
template <class Body, class Prep = NoPrep>
int host_pipeline(int ncol, int c0, int c1, int nbmax, std::vector<HostIn> &ins, std::vector<HostOut> &outs, Body body, Prep prep = Prep())
{
    std::vector<Event> tev;                  // (timing) per batch: H2D begin / end, kernels begin / end
    const int rc = host_pipeline_run(ncol, c0, c1, nbmax, ins, outs, body, prep, tev);
    if (rc != 0) {
        // An error part-way leaves up to HOST_SETS batches of DMAs and kernels in flight, some of them to and from the caller's registered
        // arrays: nothing of this call may still be running when the caller gets its error (and frees or unregisters them).
        if (G.cp_in) (void)hipStreamSynchronize(G.cp_in.get());
        if (G.stream) (void)hipStreamSynchronize(G.stream.get());
        if (G.cp_out) (void)hipStreamSynchronize(G.cp_out.get());
    }
    return rc;
}
template <class Body, class Prep>
int host_pipeline_run(int ncol, int c0, int c1, int nbmax, std::vector<HostIn> &ins, std::vector<HostOut> &outs, Body body, Prep prep, std::vector<Event> &tev)
{   // columns [c0, c1) of arrays that are ncol columns wide
    if (int rc = ensure_copy_streams()) return rc;
    // (4-byte arrays, the *_r4 entries: behind a set's float64 arrays its float32 landing area - the input rows that travel arrive there and
    // are widened into the float64 arrays, the active output rows are narrowed into it and leave from there; `land` its bytes)
    size_t set = 0, nrows = 0, out_pageable = 0, land = 0, widen_rows = 0, narrow_rows = 0;
    for (auto &a : ins) {
        set += a.h ? a.inner * a.rows * (size_t)nbmax : 0;
        nrows += a.h ? a.rows + a.inner * a.rows * (size_t)nbmax / FILL_MAX + 1 : 0;
        a.pinned = a.h && host_range_pinned(a.h, a.inner * (size_t)ncol * a.rows * a.esz);
        a.static_gen = a.h ? static_gen_of(a.h, a.inner * (size_t)ncol * a.rows * a.esz) : 0;
        if (a.h && a.esz == 4) { land += a.rows * land_stride(a.inner * (size_t)nbmax); widen_rows += a.rows; }
    }
    for (auto &a : outs) {
        set += a.rows * (size_t)nbmax;
        a.pinned = a.active && a.h && host_range_pinned(a.h, (size_t)ncol * a.rows * a.esz);
        if (a.active && a.h && !a.pinned) out_pageable += a.esz == 4 ? a.rows * land_stride((size_t)nbmax) : a.rows * (size_t)nbmax * 8;
        if (a.active && a.h && a.esz == 4) { land += a.rows * land_stride((size_t)nbmax); narrow_rows += a.rows; }
    }
    const size_t set64 = align_up(set * 8, 256);
    set = set64 + align_up(land, 256);
    if (int rc = ensure_stage(HOST_SETS * set + 4096)) return rc;
    for (auto &hs : G.hset) {
        if (int rc = ensure_hostbuf(hs.fill, nrows * sizeof(RowFill))) return rc;
        if (int rc = ensure_hostbuf(hs.out, out_pageable)) return rc;
        if (int rc = ensure_hostbuf(hs.widen, widen_rows * sizeof(RowCvt))) return rc;
        if (int rc = ensure_hostbuf(hs.narrow, narrow_rows * sizeof(RowCvt))) return rc;
    }
    auto bind = [&](int k) {                 // point the descriptors at staging set k
        double *p = (double *)(G.stage_buf.as<char>() + (size_t)k * set);
        for (auto &a : ins) { a.d = a.h ? p : nullptr; p += a.h ? a.inner * a.rows * (size_t)nbmax : 0; }
        for (auto &a : outs) { a.d = p; p += a.rows * (size_t)nbmax; }
        if (land == 0) return;
        char *q = G.stage_buf.as<char>() + (size_t)k * set + set64;
        for (auto &a : ins) { const bool on = a.h && a.esz == 4; a.land = on ? (float *)q : nullptr; q += on ? a.rows * land_stride(a.inner * (size_t)nbmax) : 0; }
        for (auto &a : outs) { const bool on = a.active && a.h && a.esz == 4; a.land = on ? (float *)q : nullptr; q += on ? a.rows * land_stride((size_t)nbmax) : 0; }
    };
    bool narrowed[HOST_SETS] = {};           // the narrow table of set k has been handed to a launch of this call
    struct Pending { bool on = false; int col0 = 0, nb = 0; } pend[HOST_SETS];
    auto copy_out = [&](int k, int col0, int nb) -> int {
        bind(k);
        HIP_TRY(hipStreamWaitEvent(G.cp_out.get(), G.ev_cmp[k].get(), 0));
        char *p = G.hset[k].out.as<char>();
        bool any = false;
        if (narrow_rows) {
            // the active float32 outputs: their staged float64 rows rounded into the landing area by one launch behind the batch's kernels
            // (the table is this set's own: the launch that read it last has ended once the D2H behind it has)
            if (narrowed[k]) HIP_TRY(hipEventSynchronize(G.ev_d2h[k].get()));
            RowCvt *ntab = G.hset[k].narrow.as<RowCvt>();
            size_t nn = 0;
            for (auto &a : outs)
                for (size_t r = 0; a.land && r < a.rows; r++) ntab[nn++] = RowCvt{a.d + (size_t)nb * r, a.land + land_stride((size_t)nb) / 4 * r, (unsigned long long)nb};
            for (size_t f0 = 0; f0 < nn; f0 += 65535)
                LAUNCH("k_narrow_rows", k_narrow_rows, dim3(cvt_blocks((size_t)nb), (unsigned)std::min<size_t>(65535, nn - f0)), dim3(256), G.cp_out.get(), (const RowCvt *)(ntab + f0));
            narrowed[k] = true;
        }
        for (auto &a : outs) {
            if (!a.active || !a.h) continue;
            if (a.esz == 4) {                // 4-byte rows out of the landing area
                const size_t st = land_stride((size_t)nb);
                if (a.pinned) { HIP_TRY(hipMemcpy2DAsync((char *)a.h + (size_t)col0 * 4, (size_t)ncol * 4, a.land, st, (size_t)nb * 4, a.rows, hipMemcpyDeviceToHost, G.cp_out.get())); continue; }
                HIP_TRY(hipMemcpyAsync(p, a.land, a.rows * st, hipMemcpyDeviceToHost, G.cp_out.get()));
                p += a.rows * st;
                any = true;
                continue;
            }
            const size_t w = (size_t)nb * 8, sp = (size_t)ncol * 8;
            if (a.pinned) { HIP_TRY(hipMemcpy2DAsync(a.h + col0, sp, a.d, w, w, a.rows, hipMemcpyDeviceToHost, G.cp_out.get())); continue; }
            HIP_TRY(hipMemcpyAsync(p, a.d, a.rows * w, hipMemcpyDeviceToHost, G.cp_out.get()));
            p += a.rows * w;
            any = true;
        }
        HIP_TRY(hipEventRecord(G.ev_d2h[k].get(), G.cp_out.get()));
        pend[k] = Pending{any, col0, nb};
        return 0;
    };
    // the pageable output arrays' rows of the batch that used set k last: pinned set -> the caller's arrays.  must = false: only if its D2H has landed
    auto unpack = [&](int k, bool must) -> int {
        if (!pend[k].on) return 0;
        if (!must) {
            const hipError_t q = hipEventQuery(G.ev_d2h[k].get());
            if (q == hipErrorNotReady) return 0;
            if (q != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        }
        pend[k].on = false;
        HIP_TRY(hipEventSynchronize(G.ev_d2h[k].get()));
        const size_t nb = (size_t)pend[k].nb, col0 = (size_t)pend[k].col0;
        struct Seg { char *dst; const char *src; size_t rows, dpitch, spitch, w; };          // (bytes: rows of 8- or of 4-byte values)
        std::vector<Seg> segs;
        size_t tot = 0, bytes = 0;
        const char *p = G.hset[k].out.as<char>();
        for (auto &a : outs) {
            if (!a.active || !a.h || a.pinned) continue;
            const size_t sp = a.esz == 4 ? land_stride(nb) : nb * 8;
            segs.push_back({(char *)a.h + col0 * a.esz, p, a.rows, (size_t)ncol * a.esz, sp, nb * a.esz});
            p += a.rows * sp;
            tot += a.rows;
            bytes += a.rows * nb * a.esz;
        }
        host_parallel(2 * bytes, [&](int t, int nt) {
            const size_t r0 = tot * (size_t)t / (size_t)nt, r1 = tot * (size_t)(t + 1) / (size_t)nt;
            size_t base = 0;
            for (auto &sg : segs) {
                const size_t a0 = std::max(r0, base), a1 = std::min(r1, base + sg.rows);
                if (a0 < a1) hostrows::copy_rows(sg.dst, sg.dpitch, sg.src, sg.spitch, sg.w, a0 - base, a1 - base);
                base += sg.rows;
            }
        });
        return 0;
    };
    StageClock clk;
    auto tmark = [&](hipStream_t st) { if (!g_stage_timing) return; Event e; (void)hipEventCreate(e.slot()); (void)hipEventRecord(e.get(), st); tev.push_back(std::move(e)); };
    const auto t_call = std::chrono::steady_clock::now();
    int i = 0, prev_col0 = 0, prev_nb = 0;
    for (int col0 = c0; col0 < c1; col0 += nbmax, i++) {
        const int nb = std::min(nbmax, c1 - col0), k = i % HOST_SETS, kprev = (i + HOST_SETS - 1) % HOST_SETS;
        bind(k);
        clk.start();
        if (i >= HOST_SETS) {
            HIP_TRY(hipStreamWaitEvent(G.cp_in.get(), G.ev_cmp[k].get(), 0));          // kernels of batch i - HOST_SETS have read staging set k
            HIP_TRY(hipEventSynchronize(G.ev_h2d[k].get()));                     // its DMAs have left the pinned set k (this thread runs ahead of the device)
            clk.lap(0);
            if (int rc = unpack(k, true)) return rc;
            clk.lap(1);
        }
        for (auto &a : ins) { a.src = a.h; a.src_ncol = (size_t)ncol; a.src_col0 = (size_t)col0; a.src_pinned = a.pinned; a.src_esz = a.esz; a.skip = nullptr; a.known = nullptr; a.known_bits = nullptr; }
        // the entry's own host work for this batch (reductions into its pinned scratch set k, which it then names as an array's source)
        if (int rc = prep(k, col0, nb, G.cp_in.get())) return rc;
        clk.lap(2);
        tmark(G.cp_in.get());
        if (int rc = stage_rows(ins, (size_t)nb, k, G.cp_in.get())) return rc;
        tmark(G.cp_in.get());
        HIP_TRY(hipEventRecord(G.ev_h2d[k].get(), G.cp_in.get()));
        clk.lap(3);
        HIP_TRY(hipStreamWaitEvent(G.stream.get(), G.ev_h2d[k].get(), 0));
        if (i >= HOST_SETS) HIP_TRY(hipStreamWaitEvent(G.stream.get(), G.ev_d2h[k].get(), 0));         // outputs of batch i - HOST_SETS have left staging set k
        tmark(G.stream.get());
        if (int rc = body(G.stream.get(), nb, col0, ins, outs)) return rc;
        tmark(G.stream.get());
        HIP_TRY(hipEventRecord(G.ev_cmp[k].get(), G.stream.get()));
        clk.lap(4);
        if (i >= 1)
            if (int rc = copy_out(kprev, prev_col0, prev_nb)) return rc;
        clk.lap(5);
        // outputs that have landed in the meantime (oldest first): unpacked now, while the device works on the batches just enqueued
        for (int j = 1; j < HOST_SETS; j++)
            if (int rc = unpack((k + j) % HOST_SETS, false)) return rc;
        clk.lap(1);
        prev_col0 = col0; prev_nb = nb;
    }
    clk.start();
    if (int rc = copy_out((i + HOST_SETS - 1) % HOST_SETS, prev_col0, prev_nb)) return rc;
    for (int j = 0; j < HOST_SETS; j++)                  // (oldest first)
        if (int rc = unpack((i + j) % HOST_SETS, true)) return rc;
    HIP_TRY(hipStreamSynchronize(G.cp_out.get()));
    HIP_TRY(hipStreamSynchronize(G.stream.get()));
    clk.lap(6);
    if (g_stage_timing) {
        double h2d = 0.0, ker = 0.0;
        for (size_t e = 0; e + 3 < tev.size(); e += 4) {
            float a = 0.f, b = 0.f;
            (void)hipEventElapsedTime(&a, tev[e].get(), tev[e + 1].get());
            (void)hipEventElapsedTime(&b, tev[e + 2].get(), tev[e + 3].get());
            h2d += a; ker += b;
        }
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        fprintf(stderr, "[rrtmg_lw_hip stage] %d columns in %d batches of <= %d: wall %.2f ms | host: wait-h2d %.2f unpack(+wait d2h) %.2f prep %.2f scan+pack+enqueue %.2f "
                        "body-enqueue %.2f copy_out-enqueue %.2f drain %.2f | device: H2D stream busy %.2f kernels %.2f\n",
                c1 - c0, i, nbmax, wall, clk.t[0], clk.t[1], clk.t[2], clk.t[3], clk.t[4], clk.t[5], clk.t[6], h2d, ker);
    }
    return 0;
}

// ---- Mersenne Twister MT19937 (Matsumoto & Nishimura 1998; init_genrand / genrand_real1 of mt19937ar) -------
// The reference's irng = 1 stream: src/mcica_random_numbers.f90:157-169 (scalar seeding), :262-295 (deviate on [0,1]).
struct MT19937 {
    uint32_t st[624];
    int cur = 624;
    explicit MT19937(uint32_t seed)
    {
        st[0] = seed;
        for (int i = 1; i < 624; i++) st[i] = 1812433253u * (st[i - 1] ^ (st[i - 1] >> 30)) + (uint32_t)i;
    }
    void refill()
    {
        for (int k = 0; k < 624; k++) {
            const uint32_t y = (st[k] & 0x80000000u) | (st[(k + 1) % 624] & 0x7fffffffu);
            st[k] = st[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        cur = 0;
    }
    double real1()
    {
        if (cur >= 624) refill();
        uint32_t y = st[cur++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return (double)y / 4294967295.0;
    }
};

// ---- chunk-start states of the Mersenne-Twister stream (k_mt_jump, mtjump.hpp) ---------------------------------------------------
// The stream of a call is NGPT slabs of `per` deviates (one sub-column each), every slab cut into M chunks of C: state (isub, m) is the
// MT19937 state isub per + m C deviates into the stream.  Two levels of doubling rounds seat them: slab starts (x^(per 2^k) applied to
// the 2^k slabs that exist), then chunk starts inside all slabs at once (x^(C 2^k)).  Cached per (seed, per), two sets (a host model that
// keeps its permuteseed pays for the jumps once; one that hands its columns over in blocks with a shorter last block alternates between
// two values of `per`).
struct MtStates {
    long long seed = -1;
    unsigned long long per = 0, C = 0;
    int M = 0;
    DevBuf dev;                         // unsigned [NGPT * M][624]
    DevBuf polys;                       // unsigned long long [32][MT_PW]
    unsigned long long used = 0;        // last use (the older set makes room)
    size_t bytes() const { return dev.bytes() + polys.bytes(); }
};
owned::NoDestroy<std::array<MtStates, 2>> g_mt_store;      // (never destroyed: see g_states)
std::array<MtStates, 2> &g_mt = g_mt_store.get();
mtj::Poly g_mt_phi{};
bool g_mt_have_phi = false;
unsigned long long g_mt_clock = 0;

int mt_states(hipStream_t s, uint32_t seed, unsigned long long per, int *M_out, unsigned long long *C_out, unsigned **dev_out)
{
    const int M = (int)std::min<unsigned long long>(512ull, std::max<unsigned long long>(1ull, (per + 65535ull) / 65536ull));   // a wavefront per chunk
    const unsigned long long C = (per + (unsigned long long)M - 1ull) / (unsigned long long)M;
    *M_out = M; *C_out = C;
    for (MtStates &S : g_mt)
        if (S.dev && S.seed == (long long)seed && S.per == per && S.M == M) { S.used = ++g_mt_clock; *dev_out = S.dev.as<unsigned>(); return 0; }
    MtStates &T = g_mt[0].used <= g_mt[1].used ? g_mt[0] : g_mt[1];
    T.used = ++g_mt_clock;
    HIP_TRY(hipDeviceSynchronize());                                // an earlier call may still be reading the states
    if (!g_mt_have_phi) {
        g_mt_phi = mtj::char_poly();
        if (!mtj::bit(g_mt_phi.data(), mtj::DEG)) return fail(RRTMG_LW_HIP_EHIP, "MT19937: characteristic polynomial not found");
        g_mt_have_phi = true;
    }
    const mtj::Poly &phi = g_mt_phi;
    const size_t need = (size_t)NGPT * M * MT_NW * sizeof(unsigned), npoly = (size_t)32 * MT_PW * sizeof(unsigned long long);
    if (int rc = grow(T.dev, need, need, "MT19937 chunk states")) return rc;
    if (int rc = grow(T.polys, npoly, npoly, "MT19937 jump polynomials")) return rc;
    T.seed = -1;
    unsigned *const st = T.dev.as<unsigned>();
    unsigned long long *const polys = T.polys.as<unsigned long long>();
    // polynomials: slab level k = 0 .. K1-1 (2^K1 >= NGPT), chunk level k = 0 .. K2-1 (2^K2 >= M)
    int K1 = 0, K2 = 0;
    while ((1 << K1) < NGPT) K1++;
    while ((1 << K2) < M) K2++;
    std::vector<unsigned long long> host((size_t)(K1 + K2) * MT_PW);
    {
        mtj::Poly p = mtj::pow_x(per, phi);
        for (int k = 0; k < K1; k++) { std::memcpy(&host[(size_t)k * MT_PW], p.data(), sizeof(p)); p = mtj::sqr_mod(p, phi); }
        if (K2) {
            p = mtj::pow_x(C, phi);
            for (int k = 0; k < K2; k++) { std::memcpy(&host[(size_t)(K1 + k) * MT_PW], p.data(), sizeof(p)); p = mtj::sqr_mod(p, phi); }
        }
    }
    HIP_TRY(hipMemcpy(polys, host.data(), host.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    {
        MT19937 mt(seed);                                           // init_genrand (src/mcica_random_numbers.f90:157-169)
        HIP_TRY(hipMemcpy(st, mt.st, sizeof(mt.st), hipMemcpyHostToDevice));
    }
    for (int k = 0; k < K1; k++) {
        const int have = 1 << k, n = std::min(have, NGPT - have);
        if (n <= 0) break;
        hipLaunchKernelGGL(k_mt_jump, dim3(n, 1), dim3(MT_BLOCK), 0, s, st, (const unsigned long long *)(polys + (size_t)k * MT_PW), 0, M, 0, have * M);
    }
    for (int k = 0; k < K2; k++) {
        const int have = 1 << k, n = std::min(have, M - have);
        if (n <= 0) break;
        hipLaunchKernelGGL(k_mt_jump, dim3(n, NGPT), dim3(MT_BLOCK), 0, s, st, (const unsigned long long *)(polys + (size_t)(K1 + k) * MT_PW), 0, 1, M, have);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "k_mt_jump launch failed: %s", hipGetErrorString(e));
    T.seed = (long long)seed; T.per = per; T.C = C; T.M = M;
    *dev_out = st;
    return 0;
}

// the table of one (draws per sub-column, permuteseed) pair: entries 0 .. KJ_NGROUP-1 jump from the seed to sub-column 8 g, the last one
// by one sub-column.  A set of them (KissTable): a host model keeps its permuteseed per call site and an averaging call its list of seeds,
// so in steady state this is a search.  A pair the set does not hold takes a slot that has never held a table - nothing reads it: its
// table is copied on the stream `s`, in front of the generator's launches, with no synchronisation - or, when all have, the slot used
// longest ago, after a device synchronisation (an earlier launch on another stream may still be reading it): a host that changes its
// seed with every call pays that synchronisation again once KISS_SLOTS pairs have been seen.  A later call that finds the table and
// launches on ANOTHER stream reads a finished copy: the copy is ordered in front of the generator of the call that made it, that call ends
// in G.ev_last, and every call waits for G.ev_last before it launches (run_pipelined, run_samples, generate_mask).
// (struct KissTable: beside State, which holds one per device)
std::atomic<long long> g_kiss_built{0};         // tables built since the library was loaded (rrtmg_lw_hip_kiss_tables_built)

int kiss_table(hipStream_t s, int stride, int permuteseed, const KissJump **dev, KissJump *jsub)
{
    KissTable &T = G.kiss;
    const long long seed = std::max(permuteseed, 0);
    constexpr size_t slot_bytes = (KJ_NGROUP + 1) * sizeof(KissJump);
    if (int rc = grow(T.dev, KISS_SLOTS * slot_bytes, KISS_SLOTS * slot_bytes, "kissvec jump tables")) return rc;
    if (int rc = grow(T.host, KISS_SLOTS * slot_bytes, KISS_SLOTS * slot_bytes, "kissvec jump tables (host)")) return rc;
    if (T.slot.empty()) T.slot.resize(KISS_SLOTS);
    KissSlot *hit = nullptr, *old = &T.slot[0];
    for (KissSlot &k : T.slot) {
        if (k.seed == seed && k.stride == (unsigned long long)stride) { hit = &k; break; }
        if (k.used < old->used) old = &k;
    }
    KissJump *const host = T.host.as<KissJump>() + (size_t)((hit ? hit : old) - &T.slot[0]) * (KJ_NGROUP + 1);
    if (!hit) {
        hit = old;
        if (hit->used != 0) HIP_TRY(hipDeviceSynchronize());
        hit->seed = -1;
        for (int g = 0; g < KJ_NGROUP; g++) host[g] = kiss_jump_entry((unsigned long long)seed + 8ull * g * (unsigned long long)stride);
        host[KJ_NGROUP] = kiss_jump_entry((unsigned long long)stride);
        HIP_TRY(hipMemcpyAsync(T.dev.as<char>() + (size_t)(hit - &T.slot[0]) * slot_bytes, host, slot_bytes, hipMemcpyHostToDevice, s));
        hit->stride = (unsigned long long)stride; hit->seed = seed;
        g_kiss_built++;
    }
    hit->used = ++T.clock;
    *dev = reinterpret_cast<const KissJump *>(T.dev.as<char>() + (size_t)(hit - &T.slot[0]) * slot_bytes);
    *jsub = host[KJ_NGROUP];
    return 0;
}

template <int RULE>
void launch_kiss_rule(hipStream_t s, const Workspace &Wk, const SubcolIn &in, const KissJump *jt, const KissJump &jsub, int ncol, int col0, int nb, int nlay)
{
    const size_t lds = (size_t)nlay * KJ_COLS * sizeof(int4);
    const dim3 grid((nb + KJ_COLS - 1) / KJ_COLS), block(KJ_BLOCK);
    hipLaunchKernelGGL(k_subcol_kiss<RULE>, grid, block, lds, s, Wk, in, jt, jsub, ncol, col0, nb, nlay);
}

// kissvec masks of columns col0 .. col0+nb-1 on stream s, from play, cldfrac and alpha `ncol` columns wide (the mask has its own width,
// Workspace::mask_stride: the columns of the call); G.W.mask must be set up (prepare_mask)
int launch_kiss(hipStream_t s, const Workspace &Wk, int ncol, int col0, int nb, int nlay, int icld, int permuteseed, const SubcolIn &in)
{
    if (icld < 1 || icld > 5) return fail(RRTMG_LW_HIP_EARG, "the sub-column generator needs icld 1..5");
    const int stride = icld == 3 ? 1 : ((icld == 4 || icld == 5) ? 2 * nlay : nlay);    // draws per sub-column (:475-530)
    const KissJump *jt = nullptr;
    KissJump jsub;
    if (int rc = kiss_table(s, stride, permuteseed, &jt, &jsub)) return rc;
    State::ProfRec r{"k_subcol_kiss", {}, {}};
    if (G.profile) { r.a = get_event(); r.b = get_event(); (void)hipEventRecord(r.a.get(), s); }
    switch (icld) {
    case 1: launch_kiss_rule<1>(s, Wk, in, jt, jsub, ncol, col0, nb, nlay); break;
    case 2: launch_kiss_rule<2>(s, Wk, in, jt, jsub, ncol, col0, nb, nlay); break;
    case 3: launch_kiss_rule<3>(s, Wk, in, jt, jsub, ncol, col0, nb, nlay); break;
    default: launch_kiss_rule<4>(s, Wk, in, jt, jsub, ncol, col0, nb, nlay); break;
    }
    if (G.profile) { (void)hipEventRecord(r.b.get(), s); G.prof.push_back(std::move(r)); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "k_subcol_kiss launch failed: %s", hipGetErrorString(e));
    return 0;
}

// mask buffer for all `ncol` columns of the call + argument checks of the generator
int prepare_mask(int ncol, int nlay, int icld, int irng, const double *alpha)
{
    if (nlay < 4 && irng == 0) return fail(RRTMG_LW_HIP_EARG, "the kissvec generator needs at least four layers");
    if ((icld == 4 || icld == 5) && !alpha) return fail(RRTMG_LW_HIP_EARG, "icld = 4/5 needs alpha");
    if (int rc = ensure_mask(nlay, (size_t)ncol)) return rc;
    G.W.mask = G.mask.as<unsigned>();
    G.W.mask_stride = (size_t)ncol;
    G.W.mask_col0 = 0;
    G.W.err = G.d_err.as<int>();
    if (irng == 0) {
        const size_t lds = (size_t)nlay * KJ_COLS * sizeof(int4);
        // (+ 64: the kernel's few bytes of static LDS count against the same limits)
        if (lds + 64 > 160 * 1024) return fail(RRTMG_LW_HIP_EARG, "nlay=%d exceeds the generator's LDS budget", nlay);
        if (lds + 64 > 48 * 1024) {
            HIP_TRY(hipFuncSetAttribute((const void *)k_subcol_kiss<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_TRY(hipFuncSetAttribute((const void *)k_subcol_kiss<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_TRY(hipFuncSetAttribute((const void *)k_subcol_kiss<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_TRY(hipFuncSetAttribute((const void *)k_subcol_kiss<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
    }
    return 0;
}

// Sub-column masks of all `ncol` columns into G.mask (device arrays play, cldfrac, alpha are (ncol,nlay)).
int generate_mask(hipStream_t s, int ncol, int nlay, int icld, int permuteseed, int irng, const double *play,
                  const double *cldfrac, const double *alpha)
{
    if (int rc = prepare_mask(ncol, nlay, icld, irng, alpha)) return rc;
    // the mask buffer is shared with an earlier device-entry call that may still be running on another stream
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));
    SubcolIn in{play, cldfrac, alpha};
    if (irng == 0) {
        if (int rc = launch_kiss(s, G.W, ncol, 0, ncol, nlay, icld, permuteseed, in)) return rc;
    } else {
        // one stream over (sub-column, column, layer): drawn chunk-parallel on the device (mt_states), applied per sub-column slab
        HIP_TRY(hipMemsetAsync(G.mask.get(), 0, (size_t)KJ_NWORD * nlay * ncol * sizeof(unsigned), s));
        const int nd = (icld == 4 || icld == 5) ? 2 : 1;
        const unsigned long long per = icld == 3 ? (unsigned long long)ncol : (unsigned long long)ncol * nlay * nd;
        int M = 0;
        unsigned long long C = 0;
        unsigned *states = nullptr;
        if (int rc = mt_states(s, (uint32_t)permuteseed, per, &M, &C, &states)) return rc;
        // as many slabs per launch as fit a 512 MB buffer of deviates (a single slab if it is larger): a small call's 140 slabs are a few launches instead of 140, a large
        // one's launches hold enough chunks (one wavefront each) to fill the device
        const int ns = (int)std::max<unsigned long long>(1ull, std::min<unsigned long long>((unsigned long long)NGPT, (512ull << 20) / (per * 8ull)));     // slabs per pass: at most 512 MB of deviates
        const size_t need = (size_t)ns * per * 8;
        if (int rc = grow(G.d_rnd, need, need, "MT19937 deviates")) return rc;
        const dim3 block(BLOCK);
        for (int isub = 0; isub < NGPT; isub += ns) {
            const int n = std::min(ns, NGPT - isub);
            hipLaunchKernelGGL(k_mt_fill, dim3(M, n), dim3(MT_BLOCK), 0, s, (const unsigned *)states, G.d_rnd.as<double>(), isub * M, M, C, per);
            hipLaunchKernelGGL(k_subcol_slab, dim3((ncol + BLOCK - 1) / BLOCK, (n + SLAB_GROUP - 1) / SLAB_GROUP), block, 0, s, G.W, in, G.d_rnd.as<const double>(), ncol, nlay, icld, isub, n, per);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "generator launch failed: %s", hipGetErrorString(e));
    return 0;
}

int check_subcol_args(int ncol, int nlay, int icld, int *irng)
{
    if (int rc = check_common(ncol, nlay)) return rc;
    if (!irng) return fail(RRTMG_LW_HIP_EARG, "irng is null");
    if (icld < 0 || icld > 5) return fail(RRTMG_LW_HIP_EPHYSICS, "MCICA_SUBCOL: INVALID ICLD");   // src/mcica_subcol_gen_lw.f90:266
    if (*irng != 0) *irng = 1;                                                                    // :442
    return 0;
}

}  // namespace

extern "C" {

const char *rrtmg_lw_hip_last_error(void)
{
    if (tl_err.empty()) { std::lock_guard<std::mutex> lk(g_lasterr_mu); tl_err = g_lasterr; }
    return tl_err.c_str();
}

static int init_state(const char *static_tables_path, const char *kdata_path, double cpdair, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(RRTMG_LW_HIP_ENODEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(RRTMG_LW_HIP_EARG, "device %d out of range (0..%d)", device, ndev - 1);
    if (!static_tables_path || !kdata_path) return fail(RRTMG_LW_HIP_EARG, "null table path");
    std::string err;
    if (!build_tables(static_tables_path, kdata_path, cpdair, G.H, err)) return fail(RRTMG_LW_HIP_EDATA, "%s", err.c_str());
    if (G.init) {
        // a re-initialisation: the graphs of small calls hold the tables of the previous one by value (heatfac, the pointers to d_ktab /
        // d_stat freed below) and the workspace freed below - none survives, whatever addresses the allocations that follow come back with
        (void)hipSetDevice(G.device);
        (void)hipDeviceSynchronize();
        graphs_clear();
        // (the *_as entries' staging is rebuilt by the next such call, on the device of this initialisation)
        G.form_buf.reset();
        G.form_gen.reset();
        if (G.device != device) G.cap.reset();       // (the capture stream belongs to the device it was made on)
    }
    static unsigned long long init_count = 0;
    G.init_gen = ++init_count;
    HIP_TRY(hipSetDevice(device));
    G.device = device;                  // (from here on the state owns resources on this device: finalize_state releases them there)
    G.sweep_attrs = false;
    G.d_ktab.reset();                   // (the tables of an earlier initialisation are never reused, whatever their size)
    G.d_stat.reset();
    if (int rc = grow(G.d_ktab, G.H.ktab.size() * 8, G.H.ktab.size() * 8, "k tables")) return rc;
    if (int rc = grow(G.d_stat, G.H.stat.size() * 8, G.H.stat.size() * 8, "static tables")) return rc;
    if (int rc = bounce_h2d(G.d_ktab.get(), G.H.ktab.data(), G.H.ktab.size() * 8)) return rc;          // (never a pageable pointer to the runtime: bounce_h2d)
    if (int rc = bounce_h2d(G.d_stat.get(), G.H.stat.data(), G.H.stat.size() * 8)) return rc;
    if (int rc = grow(G.d_err, sizeof(int), sizeof(int), "error word")) return rc;
    HIP_TRY(hipMemset(G.d_err.get(), 0, sizeof(int)));
    if (!G.stream) { if (int rc = make_stream(G.stream, 0, 0)) return rc; }
    HIP_TRY(hipDeviceGetAttribute(&G.cu_total, hipDeviceAttributeMultiprocessorCount, device));
    DevTables &D = G.D;
    D.ktab = G.d_ktab.as<double>();
    D.stat = G.d_stat.as<double>();
    for (int b = 0; b < NBND; b++) {
        D.band[b] = G.H.band[b];
        D.delwave[b] = G.H.delwave[b];
        for (int k = 0; k < 6; k++) D.refrat[b][k] = G.H.refrat[b][k];
    }
    D.sl = G.H.sl;
    D.absice0[0] = G.H.absice0[0]; D.absice0[1] = G.H.absice0[1];
    D.abscld1 = G.H.abscld1; D.absliq0 = G.H.absliq0;
    D.heatfac = G.H.heatfac; D.fluxfac = G.H.fluxfac; D.oneminus = G.H.oneminus; D.bpade = G.H.bpade;
    if (G.ws_buf) { G.ws_buf.reset(); G.ws = {}; }
    G.device = device;
    G.n1 = false;
    G.init = true;
    G.err.clear();
    tl_err.clear();
    return 0;
}

static void finalize_state();

// What this library was built with (kernels.hip, "Build switches"): bit 0 tuning build (the benchmark's kernels only), 3 the 256-g-point
// configuration, 4 kernel-geometry switches; 1 and 2 (knock-out, numerics variant) reserved, no longer set.  The shipped libraries: 0 and 8.
unsigned rrtmg_lw_hip_build_flags(void) { return BUILD_FLAGS; }

int rrtmg_lw_hip_init(const char *static_tables_path, const char *kdata_path, double cpdair, int device)
{
    return rrtmg_lw_hip_init_devices(static_tables_path, kdata_path, cpdair, 1, &device);
}

// Several GPUs from one process: state d drives devices[d].  The host-pointer entries rrtmg_lw_hip_run_nomcica / _run_mcica split
// their columns into ndev contiguous blocks, one host thread and one device (its own PCIe link, copy streams, workspace) per block; the
// device-pointer entries, the queue and the sub-column generator stay on devices[0].
int rrtmg_lw_hip_init_devices(const char *static_tables_path, const char *kdata_path, double cpdair, int ndev, const int *devices)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_cur = &g_states[0];
    if (ndev < 1 || ndev > MAXDEV || !devices) return fail(RRTMG_LW_HIP_EARG, "ndev must be 1..%d", MAXDEV);
    int rc = 0, done = 0;
    std::string err;
    for (int d = 0; d < ndev && rc == 0; d++) {
        g_cur = &g_states[d];
        rc = init_state(static_tables_path, kdata_path, cpdair, devices[d]);
        if (rc != 0) err = G.err; else done = d + 1;
    }
    if (rc == 0) {
        for (int d = ndev; d < g_ndev; d++) { g_cur = &g_states[d]; finalize_state(); }      // the surplus states of an earlier, larger set: dropped once the new set stands
        g_ndev = ndev;
    } else {
        // nothing half-initialised stays behind: every state this call touched is released (the failed one may hold tables), as are the
        // states of the earlier set - a failed init leaves the library uninitialised, and says so
        for (int d = std::max(g_ndev, done + 1) - 1; d >= 0; d--) { g_cur = &g_states[d]; G.init = G.init || G.d_ktab || G.d_stat || G.d_err || G.stream; finalize_state(); }
        g_ndev = 1;
        g_states[0].err = err;
        tl_err = err;
    }
    g_cur = &g_states[0];
    (void)hipSetDevice(g_states[0].device >= 0 ? g_states[0].device : 0);
    return rc;
}

int rrtmg_lw_hip_num_devices(void) { return g_states[0].init ? g_ndev : 0; }

int rrtmg_lw_hip_kdata_is_standin(void) { return G.init ? (G.H.standin ? 1 : 0) : -1; }

void rrtmg_lw_hip_finalize(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    for (int d = g_ndev - 1; d >= 0; d--) { g_cur = &g_states[d]; finalize_state(); }
    g_cur = &g_states[0];
    g_ndev = 1;
}

static void finalize_state()
{
    if (!G.init) return;
    const bool first = g_cur == &g_states[0];
    (void)hipSetDevice(G.device);
    (void)hipDeviceSynchronize();
    graphs_clear();
    if (first) {            // the queue and the generator's caches live on the first device
        if (Q.pinned) forget_pinned(Q.pinned.get());
        Q = ChunkQueue{};
        { std::lock_guard<std::mutex> lk(g_scan_mu); g_scan.clear(); }
        g_static.clear();
        for (MtStates &S : g_mt) S = MtStates{};
    }
    G = State();
}

// the columns per internal batch in force for a call of nlay layers (first state): the default by the call's layers or the size named
// with rrtmg_lw_hip_set_batch, halved until the sweeps' row offsets stay inside their buffer descriptors (eff_batch)
int rrtmg_lw_hip_effective_batch(int nlay)
{
    std::lock_guard<std::mutex> lk(g_mu);
    State *keep = g_cur;
    g_cur = &g_states[0];
    const int b = eff_batch(nlay < 1 ? 1 : nlay);
    g_cur = keep;
    return b;
}

int rrtmg_lw_hip_set_batch(int ncol_batch)
{
    if (ncol_batch == 0) {              // back to the default: by the call's layers (auto_batch)
        for (int d = 0; d < MAXDEV; d++) { g_states[d].batch = DEFAULT_BATCH; g_states[d].batch_set = false; }
        return 0;
    }
    if (ncol_batch < 64) return fail(RRTMG_LW_HIP_EARG, "batch must be >= 64 columns");
    if (ncol_batch > 64 * SORT_MAXBLK) return fail(RRTMG_LW_HIP_EARG, "batch must be <= %d columns", 64 * SORT_MAXBLK);      // k_blocksort orders a batch's 64-column blocks in LDS
    for (int d = 0; d < MAXDEV; d++) { g_states[d].batch = ncol_batch; g_states[d].batch_set = true; }
    return 0;
}

#ifdef RRLW_DBG_DUMP
#ifndef RRLW_TUNE
#error "RRLW_DBG_DUMP belongs to tuning builds (-DRRLW_TUNE)"
#endif
// debugging build only (tools/dbg_codes.py): the cell codes / binary-key words k_layer left in the scratch set 0 (which: 0 gas codes, 1 total codes, 2 fw); info = {ncolb, nlay}
int rrtmg_lw_hip_debug_scratch(int which, void *dst, size_t bytes, int *info)
{
    ENTRY_LOCK;
    HIP_TRY(hipDeviceSynchronize());
    info[0] = G.ws.ncolb; info[1] = G.ws.nlay;
    const void *src = which == 2 ? (const void *)G.scrset[0].fw : (const void *)G.scrset[0].scr[which == 1 ? S_CODET : S_CODE];
    const size_t have = which == 2 ? (size_t)NFW * G.ws.nlay * G.ws.ncolb * 4 : (size_t)NQUAD * G.ws.nlay * G.ws.ncolb * CODE_BYTES;
    HIP_TRY(hipMemcpy(dst, src, std::min(bytes, have), hipMemcpyDeviceToHost));
    return 0;
}
#endif

#ifdef RRLW_LAYER_STAMPS
// diagnostic build only: the cycle sums of k_layer's segments (kernels.hip, STAMP) since the last call; out[NSTAMP] = waves counted
int rrtmg_lw_hip_debug_stamps(unsigned long long *out, int n)
{
    ENTRY_LOCK;
    unsigned long long h[NSTAMP + 1] = {};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_stamps), sizeof h));
    for (int i = 0; i < n && i <= NSTAMP; i++) out[i] = h[i];
    unsigned long long z[NSTAMP + 1] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z));
    return 0;
}
#endif

int rrtmg_lw_hip_set_overlap(int on)
{
    ENTRY_LOCK;
    for (int d = 0; d < MAXDEV; d++) g_states[d].split_sweep = on != 0;       // the second scratch set is allocated by the next call that needs it
    return 0;
}

// Cloudy batches of up to `ncol` columns take ONE sweep launch per band group (the cloud-zone kernel over all levels) instead of three
// (one_sweep, above); 0 = never.  Results do not depend on it.  Returns the previous value.
int rrtmg_lw_hip_set_one_sweep_max(int ncol)
{
    ENTRY_LOCK;
    const int prev = g_one_sweep_max;
    g_one_sweep_max = ncol < 0 ? 0 : ncol;
    return prev;
}

// Device-resident one-batch calls of up to `ncol` columns are replayed as one graph from their third occurrence on (run_pipelined);
// 0 = never.  Results do not depend on it.  Returns the previous value.
int rrtmg_lw_hip_set_graph_max(int ncol)
{
    ENTRY_LOCK;
    const int prev = g_graph_max;
    g_graph_max = ncol < 0 ? 0 : ncol;
    return prev;
}
// graphs captured / calls replayed from a graph since the library was initialised (first device)
void rrtmg_lw_hip_graph_stats(long long *captures, long long *replays)
{
    ENTRY_LOCK;
    if (captures) *captures = g_states[0].graph_captures;
    if (replays) *replays = g_states[0].graph_replays;
}
// jump tables of the kissvec generator built so far (kiss_table): does not move in steady state
long long rrtmg_lw_hip_kiss_tables_built(void) { return g_kiss_built.load(); }

// Batches of up to `ncol` columns are swept one band per workgroup (g_split_max); 0 = never.  Results do not depend on it.  Returns the
// previous value.
int rrtmg_lw_hip_set_split_max(int ncol)
{
    ENTRY_LOCK;
    const int prev = g_split_max;
    g_split_max = ncol < 0 ? 0 : ncol;
    return prev;
}

// k_layer's second pass with the wide staging window for (window, layer) pairs whose columns lie more than one reference-pressure plane
// apart (terrain-following grids): on = 1 (default) / off = 0.  Results do not depend on it.  Returns the previous value.
int rrtmg_lw_hip_set_wide_window(int on)
{
    ENTRY_LOCK;
    const int prev = g_wide_window ? 1 : 0;
    g_wide_window = on != 0;
    return prev;
}

// k_layer's sixteen bands of a (window of 256 columns, layer) over two or four workgroups where the batch has too few such pairs to fill the
// chip (up to ~2 000 columns of 72 layers): on = 1 (default) / off = 0.  Results do not depend on it.  Returns the previous value.
int rrtmg_lw_hip_set_layer_split(int on)
{
    ENTRY_LOCK;
    const int prev = g_layer_split ? 1 : 0;
    g_layer_split = on != 0;
    return prev;
}

// The columns of a cloudy non-McICA batch are taken in k_colsort's order (by cloud top within windows of 256 columns): on = 1 / off = 0.
// min_gain >= 0: the block-levels a window's reordering must take out of the cloud zone (k_colsort; < 0 keeps the value).
// Results do not depend on it.  Returns the previous value.
int rrtmg_lw_hip_set_column_sort(int on, int min_gain)
{
    ENTRY_LOCK;
    const int prev = g_colsort ? 1 : 0;
    g_colsort = on != 0;
    if (min_gain >= 0) g_colsort_min = std::min(min_gain, COLSORT_NEVER);      // (k_colsort compares gain x 4 with min_gain x 4 in 32 bits)
    return prev;
}

// the threshold in force (rrtmg_lw_hip_set_column_sort's min_gain): what a caller that changes it for a while puts back
int rrtmg_lw_hip_column_sort_min(void)
{
    ENTRY_LOCK;
    return g_colsort_min;
}

// What a block that k_colsort's order leaves without any cloud adds to its window's gain, in per cent of nlay block-levels (0 .. 1000;
// such a block leaves the cloudy launches where its group of sorted blocks is cloud-free).  Results do not depend on it.  Returns the
// previous value.
int rrtmg_lw_hip_set_column_sort_clear(int percent)
{
    ENTRY_LOCK;
    const int prev = g_colsort_clear;
    g_colsort_clear = std::max(0, std::min(percent, COLSORT_CLEAR_MAX));
    return prev;
}
int rrtmg_lw_hip_column_sort_clear(void)
{
    ENTRY_LOCK;
    return g_colsort_clear;
}

// Cloud-free block groups of a cloudy batch in one k_sweepc<., 0> launch (on = 1, default) or in the three cloudy launches like every
// other group (0).  Results do not depend on it.  Returns the previous value.
int rrtmg_lw_hip_set_clear_groups(int on)
{
    ENTRY_LOCK;
    const int prev = g_clear_groups ? 1 : 0;
    g_clear_groups = on != 0;
    return prev;
}

// CU partition of the overlapped pipeline (device-pointer entries): k_layer of batch i + 1 on `layer_cus` CUs (rounded to a multiple of 8:
// the same number from every XCD), the sweeps and k_flux of batch i on the others; 0 = no partition.  A value > 0 switches the overlap on.
int rrtmg_lw_hip_set_cu_partition(int layer_cus)
{
    ENTRY_LOCK;
    if (!G.init) return fail(RRTMG_LW_HIP_ENOTINIT, "rrtmg_lw_hip_init has not been called");
    State *const keep = g_cur;
    int rc = 0;
    for (int d = 0; d < g_ndev && rc == 0; d++) {
        g_cur = &g_states[d];
        (void)hipSetDevice(G.device);
        (void)hipDeviceSynchronize();
        int n = layer_cus <= 0 ? 0 : std::max(8, std::min(G.cu_total - 8, (layer_cus + 4) / 8 * 8));
        if (G.cu_total < 16) n = 0;
        G.swset[1] = {};
        G.lay_u.reset();
        G.lay_m.reset();
        G.cu_layer = n;
        if (n > 0) {
            G.split_sweep = true;
            // (created here so that a refusal of CU masks by the runtime is reported by this call)
            if ((rc = make_stream(G.lay_u, 0, 0)) == 0 && (rc = make_stream(G.lay_m, 0, n)) == 0) rc = ensure_sweep_set(1);
            if (rc != 0 && d > 0) g_states[0].err = G.err;
        }
    }
    g_cur = keep;
    (void)hipSetDevice(G.device);
    return rc;
}
int rrtmg_lw_hip_cu_partition(void) { return g_states[0].cu_layer; }

// measurement only (tools/n1_expf_measure.sh, the prototype's GPU test): cloud-free GCM calls take k_n1 instead of the production sweeps.
// An explicit call, not an environment variable: a stray variable in a job's environment must not change the numerical path.
int rrtmg_lw_hip_set_n1_prototype(int on)
{
    ENTRY_LOCK;
    G.n1 = on != 0;
    return 0;
}
int rrtmg_lw_hip_n1_prototype(void) { return g_states[0].n1 ? 1 : 0; }

// device memory the library holds right now, over all its devices: workspaces, host-entry staging, sub-column masks, the slab buffer and
// the cached chunk states of the Mersenne-Twister stream, the kissvec jump table
long long rrtmg_lw_hip_workspace_bytes(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    size_t tot = 0;
    for (int d = 0; d < g_ndev; d++) {
        const State &S = g_states[d];
        tot += S.ws_buf.bytes() + S.opt_buf.bytes() + S.stage_buf.bytes() + S.form_buf.bytes() + S.form_gen.bytes() + S.mask.bytes() + S.d_rnd.bytes() + S.kiss.dev.bytes();
    }
    for (const MtStates &M : g_mt) tot += M.bytes();
    return (long long)tot;
}
int rrtmg_lw_hip_num_chunks(void) { return NQUAD; }
int rrtmg_lw_hip_gpoints(void) { return NGPT; }

void rrtmg_lw_hip_profile_begin(void)
{
    ENTRY_LOCK;
    for (auto &r : G.prof) { G.evpool.push_back(std::move(r.a)); G.evpool.push_back(std::move(r.b)); }
    G.prof.clear();
    G.profile = true;
}

// Stops event collection, synchronises the device and writes one line per kernel name:
// "<name> <launches> <total_ms>\n".  Returns the number of bytes written (truncated to len-1).
int rrtmg_lw_hip_profile_end(char *buf, int len)
{
    ENTRY_LOCK;
    G.profile = false;
    (void)hipDeviceSynchronize();
    std::vector<std::string> names;
    std::vector<double> total;
    std::vector<int> count;
    for (auto &r : G.prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a.get(), r.b.get()) != hipSuccess) ms = 0.f;
        size_t k = 0;
        for (; k < names.size(); k++) if (names[k] == r.name) break;
        if (k == names.size()) { names.push_back(r.name); total.push_back(0.0); count.push_back(0); }
        total[k] += ms;
        count[k] += 1;
        G.evpool.push_back(std::move(r.a));
        G.evpool.push_back(std::move(r.b));
    }
    G.prof.clear();
    std::string out;
    for (size_t k = 0; k < names.size(); k++) {
        char line[160];
        snprintf(line, sizeof line, "%s %d %.6f\n", names[k].c_str(), count[k], total[k]);
        out += line;
    }
    if (buf && len > 0) {
        const size_t n = std::min(out.size(), (size_t)len - 1);
        memcpy(buf, out.data(), n);
        buf[n] = 0;
        return (int)n;
    }
    return 0;
}

int rrtmg_lw_hip_check(void *stream)
{
    ENTRY_LOCK;
    if (!G.init) return fail(RRTMG_LW_HIP_ENOTINIT, "rrtmg_lw_hip_init has not been called");
    if (g_ndev <= 1) return read_physics_error((hipStream_t)stream);
    // several states (rrtmg_lw_hip_init_devices): the device-pointer entries run on the state of the arrays' device - wait for the stream,
    // then look at every state's error word (the first error found is reported)
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    State *const keep = g_cur;
    int rc = 0;
    for (int d = 0; d < g_ndev && rc == 0; d++) {
        g_cur = &g_states[d];
        if (!G.init) continue;
        DeviceGuard dg2;
        rc = read_physics_error(nullptr);
        if (rc != 0 && d > 0) { const std::string e = G.err; g_cur = keep; G.err = e; }
    }
    g_cur = keep;
    return rc;
}
// the state (index into the devices of rrtmg_lw_hip_init_devices) this thread's last device-pointer entry ran on
int rrtmg_lw_hip_last_device_state(void) { return tl_dev_state; }

static int nomcica_device(const CallDesc &d, const GcmIn &g, const FluxOut &out, void *stream)
{
    ENTRY_LOCK_FOR(g.play);
    if (int rc = check_call(d, out)) return rc;
    const int mode = *d.icld == 0 ? 0 : (*d.icld == 1 ? 1 : 2);      // :546-560 (icld=0 -> rtrnmr clear branch)
    const int nbmax = balanced_batch(d.ncol, eff_batch(d.nlay));
    if (int rc = ensure_workspace(d.nlay, nbmax, mode != 0, false, d.idrv, mode)) return rc;
    return run_pipelined((hipStream_t)stream, batch_of(d, mode), g, out);
}

#define GCM_PARAMS                                                                                              \
    const double *play, const double *plev, const double *tlay, const double *tlev, const double *tsfc,         \
    const double *h2ovmr, const double *o3vmr, const double *co2vmr, const double *ch4vmr, const double *n2ovmr, \
    const double *o2vmr, const double *cfc11vmr, const double *cfc12vmr, const double *cfc22vmr,               \
    const double *ccl4vmr, const double *emis
#define OUT_PARAMS                                                                                              \
    double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc, double *duflx_dt, double *duflxc_dt
#define CLOUD_PARAMS                                                                                            \
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp, const double *reice, const double *reliq
#define NOMCICA_PARAMS                                                                                          \
    int ncol, int nlay, int *icld, int idrv, GCM_PARAMS, int inflglw, int iceflglw, int liqflglw, CLOUD_PARAMS, const double *tauaer, OUT_PARAMS
#define SPEC_PARAMS double *uflxs, double *dflxs, double *uflxcs, double *dflxcs
// ... and the same names as initialisers of GcmIn{GCM_NAMES, CLOUD_NAMES, tauaer} and FluxOut{OUT_NAMES[, SPEC_NAMES]}: an entry fills them once
#define GCM_NAMES play, plev, tlay, tlev, tsfc, h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr, emis
#define CLOUD_NAMES cldfr, taucld, cicewp, cliqwp, reice, reliq
#define OUT_NAMES uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt
#define SPEC_NAMES nullptr, nullptr, uflxs, dflxs, uflxcs, dflxcs          /* (fnet, fnetc: the column entry's) */
// ... and with float arrays (the *_r4 entries); AS_: an array of another element type as the address GcmIn / FluxOut carry
#define GCM_PARAMS_R4                                                                                           \
    const float *play, const float *plev, const float *tlay, const float *tlev, const float *tsfc,              \
    const float *h2ovmr, const float *o3vmr, const float *co2vmr, const float *ch4vmr, const float *n2ovmr,     \
    const float *o2vmr, const float *cfc11vmr, const float *cfc12vmr, const float *cfc22vmr,                    \
    const float *ccl4vmr, const float *emis
#define OUT_PARAMS_R4                                                                                           \
    float *uflx, float *dflx, float *hr, float *uflxc, float *dflxc, float *hrc, float *duflx_dt, float *duflxc_dt
#define CLOUD_PARAMS_R4                                                                                         \
    const float *cldfr, const float *taucld, const float *cicewp, const float *cliqwp, const float *reice, const float *reliq
#define NOMCICA_PARAMS_R4                                                                                       \
    int ncol, int nlay, int *icld, int idrv, GCM_PARAMS_R4, int inflglw, int iceflglw, int liqflglw, CLOUD_PARAMS_R4, const float *tauaer, OUT_PARAMS_R4
#define AS_(name) (const double *)name
#define GCM_NAMES_AS                                                                                            \
    AS_(play), AS_(plev), AS_(tlay), AS_(tlev), AS_(tsfc), AS_(h2ovmr), AS_(o3vmr), AS_(co2vmr), AS_(ch4vmr), AS_(n2ovmr), AS_(o2vmr), \
    AS_(cfc11vmr), AS_(cfc12vmr), AS_(cfc22vmr), AS_(ccl4vmr), AS_(emis)
#define CLOUD_NAMES_AS AS_(cldfr), AS_(taucld), AS_(cicewp), AS_(cliqwp), AS_(reice), AS_(reliq)
#define OUT_NAMES_AS (double *)uflx, (double *)dflx, (double *)hr, (double *)uflxc, (double *)dflxc, (double *)hrc, (double *)duflx_dt, (double *)duflxc_dt

int rrtmg_lw_hip_run_nomcica_device(NOMCICA_PARAMS, void *stream)
{
    return nomcica_device({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}, {GCM_NAMES, CLOUD_NAMES, tauaer}, {OUT_NAMES}, stream);
}
int rrtmg_lw_hip_run_nomcica_spectral_device(NOMCICA_PARAMS, SPEC_PARAMS, void *stream)
{
    return nomcica_device(spectral({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}), {GCM_NAMES, CLOUD_NAMES, tauaer}, {OUT_NAMES, SPEC_NAMES}, stream);
}

}   // extern "C"

namespace {
// columns [c0, c1) of the caller's host arrays (ncol columns wide) on the calling thread's current device state; no lock taken
int nomcica_host_range(const CallDesc &d, int icld, int c0, int c1, const GcmIn &g, const FluxOut &o)
{
    const int ncol = d.ncol, nlay = d.nlay, idrv = d.idrv;
    if (int rc = check_common(ncol, nlay)) return rc;
    HIP_TRY(hipDeviceSynchronize());        // asynchronous device-entry work of earlier calls shares the workspace
    const int mode = icld == 0 ? 0 : (icld == 1 ? 1 : 2);
    const bool cloud = icld >= 1;           // inatm copies the cloud arrays only when icld >= 1 (:893-910)
    // host arrays: the copies bound the rate (PCIe), and they overlap with the kernels only across batches - smaller batches than
    // the device-resident default
    const int nbmax = balanced_batch(c1 - c0, std::min(eff_batch(nlay), HOST_BATCH));
    if (int rc = ensure_workspace(nlay, nbmax, mode != 0, false, idrv, mode)) return rc;
    const size_t L = (size_t)nlay;
    // What the copies need not carry (62 % of a column's bytes are taucld and tauaer, 2 x 16 nlay values):
    //  * with inflglw >= 1 cldprop reads taucld only through the sum over the bands, tauctot (src/rrtmg_lw_cldprop.f90:173-186): the sum is
    //    formed here, in the reference's order, on the host threads - one value per (column, layer) travels instead of sixteen;
    //  * rows that hold one value for all columns of a batch - zero aerosol / cloud rows, well-mixed gases - are not copied (stage_rows).
    const bool use_tot = cloud && d.inflg != 0;
    std::vector<HostIn> ins;
    if (int rc = host_ins(ins, g, nullptr, L, cloud, use_tot ? 1 : NBND, NA_GCM, "", d.esz)) return rc;
    if (use_tot) {
        const size_t need = HOST_SETS * L * (size_t)nbmax * sizeof(double);
        if (G.h_tot && G.h_tot.bytes() < need) HIP_TRY(hipDeviceSynchronize());        // (an earlier call's copies may still read it)
        if (int rc = grow(G.h_tot, need, need, "pinned tauctot")) return rc;
    }
    std::vector<unsigned char> cloudfree(L, 0), cf_uni(L, 0);
    std::vector<uint64_t> cf_bits(L, 0);
    auto prep = [&](int k, int col0, int nb, hipStream_t) -> int {
        if (!cloud) return 0;
        if (d.esz == 4) rows_below((const float *)g.cldfr, 1, L, (size_t)ncol, (size_t)col0, (size_t)nb, 1.e-20, cloudfree.data(), cf_uni.data(), cf_bits.data());
        else rows_below(g.cldfr, 1, L, (size_t)ncol, (size_t)col0, (size_t)nb, 1.e-20, cloudfree.data(), cf_uni.data(), cf_bits.data());
        skip_cloudfree(ins, cloudfree.data(), cf_uni.data(), cf_bits.data());
        if (!use_tot) return 0;
        double *tot = G.h_tot.as<double>() + (size_t)k * L * (size_t)nbmax;        // (the pipeline has waited for the copies that read scratch set k last)
        size_t cloudy_layers = 0;
        for (size_t l = 0; l < L; l++) cloudy_layers += cloudfree[l] ? 0 : 1;
        host_parallel((size_t)NBND * cloudy_layers * (size_t)nb * d.esz, [&](int t, int nt) {
            // (pieces of 4 096 columns of a layer, dealt round-robin: the cloudy layers are few)
            const size_t piece = 4096, per = ((size_t)nb + piece - 1) / piece;
            size_t task = 0;
            for (size_t lay = 0; lay < L; lay++) {
                if (cloudfree[lay]) continue;
                for (size_t pc = 0; pc < per; pc++, task++) {
                    if (task % (size_t)nt != (size_t)t) continue;
                    const size_t c1 = std::min((size_t)nb, (pc + 1) * piece);
                    // (float bands: each widened, added in float64 in the same order - the float64 entry's sum on the widened array)
                    if (d.esz == 4) {
                        const float *p = (const float *)g.taucld + (size_t)NBND * ((size_t)col0 + pc * piece + (size_t)ncol * lay);
                        for (size_t c = pc * piece; c < c1; c++, p += NBND) tot[lay * (size_t)nb + c] = hostrows::band_sum(p, NBND);
                        continue;
                    }
                    for (size_t c = pc * piece; c < c1; c++) {
                        const double *p = g.taucld + (size_t)NBND * ((size_t)col0 + c + (size_t)ncol * lay);
                        double sum = 0.0;
                        for (int ib = 0; ib < NBND; ib++) sum = sum + p[ib];
                        tot[lay * (size_t)nb + c] = sum;
                    }
                }
            }
        });
        HostIn &tc = ins[staged_at(A_TAUCLD)];
        tc.src = tot; tc.src_ncol = (size_t)nb; tc.src_col0 = 0; tc.src_pinned = true; tc.src_esz = 8;      // rows of nb float64 sums, from the pinned scratch
        return 0;
    };
    if (!have_outs(o)) return fail(RRTMG_LW_HIP_EARG, "null output array");
    std::vector<HostOut> outs = host_outs(o, L, idrv, d.esz);
    auto body = [&](hipStream_t s, int nb, int, std::vector<HostIn> &in, std::vector<HostOut> &out_) -> int {
        GcmIn gd = staged_gcm(in);
        if (use_tot) { gd.tauctot = gd.taucld; gd.taucld = nullptr; }
        return run_batch<true>(s, staged_batch(d, mode, nb), gd, ColIn{}, staged_flux(out_));
    };
    if (int rc = host_pipeline(ncol, c0, c1, nbmax, ins, outs, body, prep)) return rc;
    hipStream_t s = G.stream.get();
    return read_physics_error(s);
}

// The columns of a host-pointer call over the devices of rrtmg_lw_hip_init_devices: contiguous blocks (multiples of 64 columns), one host
// thread per device; every block runs the one-device pipeline on its own state (H2D | kernels | D2H on that device's streams).  Columns
// are independent (src/rrtmg_lw_rad.nomcica.f90:472), so the results do not depend on the split.  Caller holds the entry lock.
template <class RangeFn>
int fan_out(int ncol, RangeFn range)
{
    State *const home = g_cur;
    if (g_ndev <= 1 || ncol < 128) return range(0, ncol);
    const int per = (int)align_up((size_t)(ncol + g_ndev - 1) / g_ndev, 64);
    int rcs[MAXDEV] = {};
    std::vector<std::thread> th;
    for (int d = 0; d < g_ndev; d++) {
        const int c0 = d * per, c1 = std::min(ncol, c0 + per);
        if (c0 >= c1) break;
        th.emplace_back([&rcs, &range, d, c0, c1]() {
            g_cur = &g_states[d];
            tl_pool = d; tl_share = g_ndev;
            if (hipSetDevice(G.device) != hipSuccess) { rcs[d] = fail(RRTMG_LW_HIP_EHIP, "hipSetDevice(%d) failed", G.device); return; }
            rcs[d] = range(c0, c1);
        });
    }
    for (auto &x : th) x.join();
    for (int d = 0; d < g_ndev; d++)
        if (rcs[d] != 0) { if (&g_states[d] != home) home->err = g_states[d].err; tl_err = g_states[d].err; return rcs[d]; }       // (the worker's thread-local text is not this thread's)
    return 0;
}

int nomcica_host(const CallDesc &d, const GcmIn &g, const FluxOut &out)
{
    if (int rc = check_call(d, out)) return rc;
    const int ic = *d.icld;
    return fan_out(d.ncol, [&](int c0, int c1) { return nomcica_host_range(d, ic, c0, c1, g, out); });
}
bool comb_enabled();
int comb_max();
long long comb_calls_total();
long long comb_passes_total();
int nomcica_combined(const CallDesc &d, const GcmIn &g, const FluxOut &out);
}   // namespace

extern "C" {

int rrtmg_lw_hip_run_nomcica(NOMCICA_PARAMS)
{
    const CallDesc d{ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw};
    const GcmIn g{GCM_NAMES, CLOUD_NAMES, tauaer};
    const FluxOut out{OUT_NAMES};
    if (ncol >= 1 && ncol <= comb_max() && icld && comb_enabled()) return nomcica_combined(d, g, out);
    ENTRY_LOCK;
    return nomcica_host(d, g, out);
}

// the same with spectral outputs; such a call does not join the combining entry (it takes the entry lock like any other call)
int rrtmg_lw_hip_run_nomcica_spectral(NOMCICA_PARAMS, SPEC_PARAMS)
{
    ENTRY_LOCK;
    return nomcica_host(spectral({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}), {GCM_NAMES, CLOUD_NAMES, tauaer}, {OUT_NAMES, SPEC_NAMES});
}

// float32 host arrays (the header's "_r4" section): the same call with 4-byte elements below the entry; takes the entry lock like the
// spectral entry, a small call does not join the combining one
int rrtmg_lw_hip_run_nomcica_r4(NOMCICA_PARAMS_R4)
{
    ENTRY_LOCK;
    return nomcica_host(real4({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}), {GCM_NAMES_AS, CLOUD_NAMES_AS, AS_(tauaer)}, {OUT_NAMES_AS});
}

// calls and device passes of the combining entry since the library was loaded (a pass serves one or more calls)
void rrtmg_lw_hip_combine_stats(long long *calls, long long *passes)
{
    if (calls) *calls = comb_calls_total();
    if (passes) *passes = comb_passes_total();
}

int rrtmg_lw_hip_run_columns(
    int ncol, int nlayers, int istart, int iend, int icld, int idrv,
    const double *pavel, const double *tavel, const double *pz, const double *tz, const double *tbound,
    const double *semiss, const double *coldry, const double *wkl, const double *wbrodl, const double *wx,
    const double *pwvcm, int inflag, int iceflag, int liqflag, const double *cldfrac, const double *tauc,
    const double *ciwp, const double *clwp, const double *rei, const double *rel, const double *taua,
    double *totuflux, double *totdflux, double *fnet, double *htr,
    double *totuclfl, double *totdclfl, double *fnetc, double *htrc,
    double *dtotuflux_dt, double *dtotuclfl_dt)
{
    ENTRY_LOCK;
    if (int rc = check_common(ncol, nlayers)) return rc;
    if (G.init) HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    if (istart < 1 || iend > 16 || istart > iend) return fail(RRTMG_LW_HIP_EARG, "bad band range %d..%d", istart, iend);
    if (ncol > eff_batch(nlayers)) return fail(RRTMG_LW_HIP_EARG, "run_columns handles at most one batch (%d columns)", eff_batch(nlayers));
    const int mode = icld == 0 ? 0 : (icld == 1 ? 1 : 2);
    if (int rc = ensure_workspace(nlayers, ncol, true, false, idrv, mode)) return rc;
    const size_t n = (size_t)ncol, L = (size_t)nlayers;
    struct In { const double *h; size_t cnt; double *d; };
    In ins[] = {{pavel, n * L, 0}, {tavel, n * L, 0}, {pz, n * (L + 1), 0}, {tz, n * (L + 1), 0}, {tbound, n, 0}, {semiss, 16 * n, 0},
                {coldry, n * L, 0}, {wkl, 7 * n * L, 0}, {wbrodl, n * L, 0}, {wx, 4 * n * L, 0}, {pwvcm, n, 0}, {cldfrac, n * L, 0},
                {tauc, 16 * n * L, 0}, {ciwp, n * L, 0}, {clwp, n * L, 0}, {rei, n * L, 0}, {rel, n * L, 0}, {taua, 16 * n * L, 0}};
    size_t tot = 0;
    for (auto &i : ins) tot += i.cnt;
    const size_t out_d = 10 * n * (L + 1);
    if (int rc = ensure_stage((tot + out_d) * 8 + 4096)) return rc;
    double *p = G.stage_buf.as<double>();
    hipStream_t s = G.stream.get();
    for (auto &i : ins) {
        i.d = p; p += i.cnt;
        if (int rc = bounce_h2d(i.d, i.h, i.cnt * 8)) return rc;
    }
    double *o[10];
    for (auto &q : o) { q = p; p += n * (L + 1); }
    ColIn c{ins[0].d, ins[1].d, ins[2].d, ins[3].d, ins[4].d, ins[5].d, ins[6].d, ins[7].d, ins[8].d, ins[9].d, ins[10].d,
            ins[11].d, ins[12].d, ins[13].d, ins[14].d, ins[15].d, ins[16].d, ins[17].d};
    GcmIn g{};
    // o: 0 uflx 1 dflx 2 fnet 3 htr 4 uclfl 5 dclfl 6 fnetc 7 htrc 8 duflx 9 duclfl ; htr arrays hold (ncol, 0:nlayers), top level = 0
    HIP_TRY(hipMemsetAsync(o[3], 0, n * (L + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(o[7], 0, n * (L + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(o[8], 0, n * (L + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(o[9], 0, n * (L + 1) * 8, s));
    FluxOut out{o[0], o[1], o[3], o[4], o[5], o[7], o[8], o[9], o[2], o[6]};
    Batch b;
    b.nlay = nlayers; b.nct = b.nb = ncol; b.mode = mode; b.idrv = idrv; b.istart = istart; b.iend = iend;
    b.inflag = inflag; b.iceflag = iceflag; b.liqflag = liqflag;
    if (int rc = run_batch<false>(s, b, g, c, out)) return rc;
    double *ho[10] = {totuflux, totdflux, fnet, htr, totuclfl, totdclfl, fnetc, htrc, dtotuflux_dt, dtotuclfl_dt};
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 10; k++) if (int rc = bounce_d2h(ho[k], o[k], n * (L + 1) * 8)) return rc;
    return read_physics_error(s);
}

// ---- gas optics and Planck sources (include/rrtmg_lw_hip.h) ---------------------------------------------------------------------------
#define OPTICS_GCM_PARAMS                                                                                       \
    int ncol, int nlay, int idrv, GCM_PARAMS,                                                                   \
    double *taug, double *fracs, double *planklay, double *planklev, double *plankbnd, double *dplankbnd_dt

// the device entry on arrays `ld` columns wide (rrtmg_lw_hip_gas_optics_device: ld = ncol; the view entry's in-place form: every pointer
// at the call's first column)
static int gas_optics_device_ld(OPTICS_GCM_PARAMS, int ld, void *stream)
{
    ENTRY_LOCK_FOR(play);
    if (int rc = check_common(ncol, nlay)) return rc;
    const OptOut o{taug, fracs, planklay, planklev, plankbnd, idrv == 1 ? dplankbnd_dt : nullptr};
    if (int rc = check_optics(idrv, o)) return rc;
    const GcmIn g{GCM_NAMES};
    const double *in[NA_IN];
    gcm_pointers(g, nullptr, in);
    for (int a = 0; a <= A_EMIS; a++) if (!in[a]) return fail(RRTMG_LW_HIP_EARG, "gas optics: null input array");
    if (int rc = ensure_pipeline()) return rc;
    const int nbmax = balanced_batch(ncol, eff_batch(nlay));
    if (int rc = ensure_optics_ws(nlay, nbmax)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the workspace
    Batch b;
    b.nlay = nlay; b.nct = ld; b.ncall = ncol; b.idrv = idrv;
    for (b.col0 = 0; b.col0 < ncol; b.col0 += nbmax) {
        b.nb = std::min(nbmax, ncol - b.col0);
        if (int rc = run_optics<true>(s, b, g, ColIn{}, o)) return rc;
    }
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return 0;
}
int rrtmg_lw_hip_gas_optics_device(OPTICS_GCM_PARAMS, void *stream)
{
    return gas_optics_device_ld(ncol, nlay, idrv, GCM_NAMES, taug, fracs, planklay, planklev, plankbnd, dplankbnd_dt, ncol, stream);
}

// columns [c0, c1) of a host-pointer gas-optics call on the calling thread's current device state (the fan-out's worker); no lock taken
static int gas_optics_host_range(int ncol, int c0, int c1, int nlay, int idrv, const GcmIn &g, const OptOut &h)
{
    HIP_TRY(hipDeviceSynchronize());        // asynchronous device-entry work of earlier calls shares the workspace
    const size_t L = (size_t)nlay;
    std::vector<HostIn> ins;
    if (int rc = host_ins(ins, g, nullptr, L, false, 0, A_EMIS + 1, "gas optics: ")) return rc;
    auto out = [](double *p, size_t rows) { return HostOut{p, p ? rows : 0, nullptr, p != nullptr}; };
    std::vector<HostOut> outs = {out(h.taug, (size_t)NGPT * L), out(h.fracs, (size_t)NGPT * L), out(h.planklay, NBND * L), out(h.planklev, NBND * (L + 1)),
                                 out(h.plankbnd, NBND), out(idrv == 1 ? h.dplankbnd : nullptr, NBND)};
    // (the outputs are ~40 times a column's inputs: batches of at most ~256 MB of staging each)
    size_t per_col = 0;
    for (auto &a : ins) per_col += a.inner * a.rows * 8;
    for (auto &a : outs) per_col += a.rows * 8;
    const int cap = std::max(256, (int)std::min<size_t>((size_t)std::min(eff_batch(nlay), HOST_BATCH), ((size_t)256 << 20) / per_col / 256 * 256));
    const int nbmax = balanced_batch(c1 - c0, cap);
    if (int rc = ensure_optics_ws(nlay, nbmax)) return rc;
    auto body = [&](hipStream_t s, int nb, int, std::vector<HostIn> &in, std::vector<HostOut> &o_) -> int {
        auto d = [&](int k) { return o_[k].active ? o_[k].d : nullptr; };
        const OptOut o{d(0), d(1), d(2), d(3), d(4), d(5)};
        Batch b;
        b.nlay = nlay; b.nct = b.nb = nb; b.idrv = idrv;
        return run_optics<true>(s, b, staged_gcm(in), ColIn{}, o);
    };
    return host_pipeline(ncol, c0, c1, nbmax, ins, outs, body);
}

int rrtmg_lw_hip_gas_optics(OPTICS_GCM_PARAMS)
{
    ENTRY_LOCK;
    if (int rc = check_common(ncol, nlay)) return rc;
    const OptOut o{taug, fracs, planklay, planklev, plankbnd, dplankbnd_dt};
    if (int rc = check_optics(idrv, o)) return rc;
    const GcmIn g{GCM_NAMES};
    return fan_out(ncol, [&](int c0, int c1) { return gas_optics_host_range(ncol, c0, c1, nlay, idrv, g, o); });
}

int rrtmg_lw_hip_gas_optics_columns(
    int ncol, int nlayers, int idrv,
    const double *pavel, const double *tavel, const double *pz, const double *tz, const double *tbound,
    const double *semiss, const double *coldry, const double *wkl, const double *wbrodl, const double *wx,
    const double *pwvcm,
    double *taug, double *fracs, double *planklay, double *planklev, double *plankbnd, double *dplankbnd_dt)
{
    ENTRY_LOCK;
    if (int rc = check_common(ncol, nlayers)) return rc;
    if (int rc = check_optics(idrv, OptOut{taug, fracs, planklay, planklev, plankbnd, dplankbnd_dt})) return rc;
    if (ncol > eff_batch(nlayers)) return fail(RRTMG_LW_HIP_EARG, "gas_optics_columns handles at most one batch (%d columns)", eff_batch(nlayers));
    HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    if (int rc = ensure_optics_ws(nlayers, ncol)) return rc;
    const size_t n = (size_t)ncol, L = (size_t)nlayers;
    struct Arr { const double *h; size_t cnt; double *d; };
    Arr ins[] = {{pavel, n * L, 0}, {tavel, n * L, 0}, {pz, n * (L + 1), 0}, {tz, n * (L + 1), 0}, {tbound, n, 0}, {semiss, 16 * n, 0},
                 {coldry, n * L, 0}, {wkl, 7 * n * L, 0}, {wbrodl, n * L, 0}, {wx, 4 * n * L, 0}, {pwvcm, n, 0}};
    struct Res { double *h; size_t cnt; double *d; };
    Res outs[] = {{taug, (size_t)NGPT * n * L, 0}, {fracs, (size_t)NGPT * n * L, 0}, {planklay, NBND * n * L, 0}, {planklev, NBND * n * (L + 1), 0},
                  {plankbnd, NBND * n, 0}, {idrv == 1 ? dplankbnd_dt : nullptr, NBND * n, 0}};
    size_t tot = 0;
    for (auto &i : ins) {
        if (!i.h) return fail(RRTMG_LW_HIP_EARG, "gas optics: null input array");
        tot += i.cnt;
    }
    for (auto &r : outs) tot += r.h ? r.cnt : 0;
    if (int rc = ensure_stage(tot * 8 + 4096)) return rc;
    double *p = G.stage_buf.as<double>();
    for (auto &i : ins) {
        i.d = p; p += i.cnt;
        if (int rc = bounce_h2d(i.d, i.h, i.cnt * 8)) return rc;
    }
    for (auto &r : outs) if (r.h) { r.d = p; p += r.cnt; }
    const ColIn c{ins[0].d, ins[1].d, ins[2].d, ins[3].d, ins[4].d, ins[5].d, ins[6].d, ins[7].d, ins[8].d, ins[9].d, ins[10].d};
    const OptOut o{outs[0].d, outs[1].d, outs[2].d, outs[3].d, outs[4].d, outs[5].d};
    const hipStream_t s = G.stream.get();
    Batch b;
    b.nlay = nlayers; b.nct = b.nb = ncol; b.idrv = idrv;
    if (int rc = run_optics<false>(s, b, GcmIn{}, c, o)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    for (auto &r : outs) if (r.h) { if (int rc = bounce_d2h(r.h, r.d, r.cnt * 8)) return rc; }
    return 0;
}

// McICA flavour of the prepared-column entry: cldprmc -> setcoef -> taumol -> rtrnmc for `ncol` (column, sample) pairs.
int rrtmg_lw_hip_run_columns_mcica(
    int ncol, int nlayers, int istart, int iend, int icld, int idrv,
    const double *pavel, const double *tavel, const double *pz, const double *tz, const double *tbound,
    const double *semiss, const double *coldry, const double *wkl, const double *wbrodl, const double *wx,
    const double *pwvcm, int inflag, int iceflag, int liqflag, const double *cldfmc, const double *taucmc,
    const double *ciwpmc, const double *clwpmc, const double *reicmc, const double *relqmc, const double *taua,
    double *totuflux, double *totdflux, double *fnet, double *htr,
    double *totuclfl, double *totdclfl, double *fnetc, double *htrc,
    double *dtotuflux_dt, double *dtotuclfl_dt)
{
    ENTRY_LOCK;
    if (int rc = check_mcica_build()) return rc;
    if (int rc = check_common(ncol, nlayers)) return rc;
    if (G.init) HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    if (istart < 1 || iend > 16 || istart > iend) return fail(RRTMG_LW_HIP_EARG, "bad band range %d..%d", istart, iend);
    if (ncol > eff_batch(nlayers)) return fail(RRTMG_LW_HIP_EARG, "run_columns_mcica handles at most one batch (%d columns)", eff_batch(nlayers));
    const int mode = icld == 0 ? 0 : 3;
    if (int rc = ensure_workspace(nlayers, ncol, true, true, idrv, mode)) return rc;
    const size_t n = (size_t)ncol, L = (size_t)nlayers;
    struct In { const double *h; size_t cnt; double *d; };
    In ins[] = {{pavel, n * L, 0}, {tavel, n * L, 0}, {pz, n * (L + 1), 0}, {tz, n * (L + 1), 0}, {tbound, n, 0}, {semiss, 16 * n, 0},
                {coldry, n * L, 0}, {wkl, 7 * n * L, 0}, {wbrodl, n * L, 0}, {wx, 4 * n * L, 0}, {pwvcm, n, 0},
                {cldfmc, NGPT * n * L, 0}, {taucmc, NGPT * n * L, 0}, {ciwpmc, NGPT * n * L, 0}, {clwpmc, NGPT * n * L, 0},
                {reicmc, n * L, 0}, {relqmc, n * L, 0}, {taua, 16 * n * L, 0}};
    size_t tot = 0;
    for (auto &i : ins) { if (!i.h) return fail(RRTMG_LW_HIP_EARG, "null input array"); tot += i.cnt; }
    const size_t out_d = 10 * n * (L + 1);
    if (int rc = ensure_stage((tot + out_d) * 8 + 4096)) return rc;
    double *p = G.stage_buf.as<double>();
    hipStream_t s = G.stream.get();
    for (auto &i : ins) {
        i.d = p; p += i.cnt;
        if (int rc = bounce_h2d(i.d, i.h, i.cnt * 8)) return rc;
    }
    double *o[10];
    for (auto &q : o) { q = p; p += n * (L + 1); }
    ColIn c{ins[0].d, ins[1].d, ins[2].d, ins[3].d, ins[4].d, ins[5].d, ins[6].d, ins[7].d, ins[8].d, ins[9].d, ins[10].d,
            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ins[17].d};
    McIn m{ins[11].d, ins[12].d, ins[13].d, ins[14].d, ins[15].d, ins[16].d};
    GcmIn g{};
    HIP_TRY(hipMemsetAsync(o[3], 0, n * (L + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(o[7], 0, n * (L + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(o[8], 0, n * (L + 1) * 8, s));
    HIP_TRY(hipMemsetAsync(o[9], 0, n * (L + 1) * 8, s));
    FluxOut out{o[0], o[1], o[3], o[4], o[5], o[7], o[8], o[9], o[2], o[6]};
    Batch b;
    b.nlay = nlayers; b.nct = b.nb = ncol; b.mode = mode; b.idrv = idrv; b.istart = istart; b.iend = iend;
    b.inflag = inflag; b.iceflag = iceflag; b.liqflag = liqflag; b.mc = &m;
    if (int rc = run_batch<false>(s, b, g, c, out)) return rc;
    double *ho[10] = {totuflux, totdflux, fnet, htr, totuclfl, totdclfl, fnetc, htrc, dtotuflux_dt, dtotuclfl_dt};
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 10; k++) if (int rc = bounce_d2h(ho[k], o[k], n * (L + 1) * 8)) return rc;
    return read_physics_error(s);
}

// Pin a host array the caller will pass repeatedly (a GCM's profile and flux arrays live for the whole run): the H2D / D2H copies
// of the host-pointer entries then run as asynchronous DMA at PCIe rate instead of through the runtime's pageable staging.
int rrtmg_lw_hip_host_register(void *ptr, long long bytes)
{
    ENTRY_LOCK;
    if (!G.init) return fail(RRTMG_LW_HIP_ENOTINIT, "rrtmg_lw_hip_init has not been called");
    if (!ptr || bytes <= 0) return fail(RRTMG_LW_HIP_EARG, "bad host range");
    HIP_TRY(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
    g_pinned.emplace_back((const char *)ptr, (size_t)bytes);
    return 0;
}

int rrtmg_lw_hip_host_is_registered(const void *ptr, long long bytes)
{
    ENTRY_LOCK;
    return (ptr && bytes > 0 && host_range_pinned(ptr, (size_t)bytes)) ? 1 : 0;
}

int rrtmg_lw_hip_host_unregister(void *ptr)
{
    ENTRY_LOCK;
    if (!ptr) return fail(RRTMG_LW_HIP_EARG, "null pointer");
    HIP_TRY(hipHostUnregister(ptr));
    forget_pinned(ptr);
    return 0;
}

// The caller declares [ptr, ptr + bytes) static: its contents stay as they are until rrtmg_lw_hip_host_changed(ptr).  The host-pointer entries
// then scan each of its rows once per column batch shape instead of once per call (g_scan).  Nothing else changes: an array that is not
// declared is scanned on every call.
int rrtmg_lw_hip_host_static(const void *ptr, long long bytes)
{
    ENTRY_LOCK;
    if (!ptr || bytes <= 0) return fail(RRTMG_LW_HIP_EARG, "bad range");
    for (auto &r : g_static)
        if (r.p == (const char *)ptr) { r.bytes = (size_t)bytes; r.gen = ++g_static_gen; return 0; }
    g_static.push_back(StaticRange{(const char *)ptr, (size_t)bytes, ++g_static_gen});
    return 0;
}
// The contents of the static range that starts at ptr have changed: its cached row scans are dropped and the next call scans it again.
// keep = 0 also withdraws the declaration (before the array is freed).
int rrtmg_lw_hip_host_changed(const void *ptr, int keep)
{
    ENTRY_LOCK;
    for (size_t i = 0; i < g_static.size(); i++) {
        if (g_static[i].p != (const char *)ptr) continue;
        const char *lo = g_static[i].p, *hi = lo + g_static[i].bytes;
        {
            std::lock_guard<std::mutex> lk(g_scan_mu);
            for (auto it = g_scan.begin(); it != g_scan.end();)
                if ((const char *)it->first.base >= lo && (const char *)it->first.base < hi) it = g_scan.erase(it); else ++it;
        }
        if (keep) g_static[i].gen = ++g_static_gen; else g_static.erase(g_static.begin() + (long)i);
        return 0;
    }
    return fail(RRTMG_LW_HIP_EARG, "no static range starts at this address");
}

// Streams `bytes` from one device buffer into another with 16 B per lane (k_calibrate): known traffic for PMC calibration.
int rrtmg_lw_hip_calibrate_stream(long long bytes)
{
    ENTRY_LOCK;
    if (!G.init) return fail(RRTMG_LW_HIP_ENOTINIT, "rrtmg_lw_hip_init has not been called");
    if (bytes < 16) return fail(RRTMG_LW_HIP_EARG, "bytes must be >= 16");
    const size_t n = (size_t)bytes / 16;
    DevBuf a, b;
    if (int rc = grow(a, n * 16, n * 16, "calibration source")) return rc;
    if (int rc = grow(b, n * 16, n * 16, "calibration target")) return rc;
    (void)hipMemset(a.get(), 0, n * 16);
    (void)hipDeviceSynchronize();
    // (through the launch wrapper: under rrtmg_lw_hip_profile_begin / _end the copy's own time is the yardstick of tools/adjust_tsfc_timing.py)
    LAUNCH("k_calibrate", k_calibrate, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), G.stream.get(), a.as<const double2>(), b.as<double2>(), n);
    hipError_t e = hipStreamSynchronize(G.stream.get());
    if (e != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "calibration kernel failed: %s", hipGetErrorString(e));
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Aggregation of small calls (include/rrtmg_lw_hip.h): chunks are recorded, packed column-wise into one pinned staging set and
// solved in one pass through the host-pointer entry.
// ---------------------------------------------------------------------------------------------------
int rrtmg_lw_hip_queue_begin(int nlay, int icld, int idrv, int inflglw, int iceflglw, int liqflglw)
{
    ENTRY_LOCK;
    if (int rc = check_common(1, nlay)) return rc;
    if (Q.open && !Q.chunks.empty()) return fail(RRTMG_LW_HIP_EARG, "%lld queued columns have not been flushed", Q.ncol);
    Q.chunks.clear();
    Q.ncol = 0;
    Q.nlay = nlay; Q.icld = icld; Q.idrv = idrv; Q.inflg = inflglw; Q.iceflg = iceflglw; Q.liqflg = liqflglw;
    Q.open = true;
    return 0;
}

int rrtmg_lw_hip_queue_columns(void) { std::lock_guard<std::mutex> lk(g_mu); return (int)Q.ncol; }

int rrtmg_lw_hip_queue_add(int ncol, int *icld, GCM_PARAMS, CLOUD_PARAMS, const double *tauaer, OUT_PARAMS)
{
    ENTRY_LOCK;
    if (!Q.open) return fail(RRTMG_LW_HIP_EARG, "rrtmg_lw_hip_queue_begin has not been called");
    if (ncol < 1) return fail(RRTMG_LW_HIP_EARG, "bad chunk size %d", ncol);
    if (icld && *icld != Q.icld) return fail(RRTMG_LW_HIP_EARG, "chunk icld %d differs from the queue's %d", *icld, Q.icld);
    const QueuedChunk c{{ncol, Q.nlay, icld, Q.idrv, Q.inflg, Q.iceflg, Q.liqflg}, {GCM_NAMES, CLOUD_NAMES, tauaer}, nullptr, {OUT_NAMES}};
    const int icld_eff = (Q.icld < 0 || Q.icld > 3) ? 2 : Q.icld;
    const double *in[NA_IN];
    gcm_pointers(c.in, nullptr, in);
    for (int a = 0; a < NA_GCM; a++)              // inatm reads the cloud arrays only when icld >= 1
        if (!in[a] && !(CALL_ARRAYS[a].cloud && icld_eff == 0)) return fail(RRTMG_LW_HIP_EARG, "null input array (argument %d)", a);
    if (!have_outs(c.out)) return fail(RRTMG_LW_HIP_EARG, "null output array");
    if (Q.idrv == 1 && (!duflx_dt || !duflxc_dt)) return fail(RRTMG_LW_HIP_EARG, "idrv=1 needs duflx_dt and duflxc_dt");
    if (Q.ncol + ncol > 0x7fffffffLL) return fail(RRTMG_LW_HIP_EARG, "too many queued columns");
    Q.chunks.push_back(c);
    Q.ncol += ncol;
    return 0;
}

}   // extern "C"

// f(i) for i in [0, n) on up to 8 host threads (contiguous index ranges)
template <class F>
static void queue_parallel(size_t n, F f)
{
    // (on the persistent host threads: a pass of the combining entry packs sixteen chunks, and eight thread starts cost more than that)
    if (n < 4) { for (size_t i = 0; i < n; i++) f(i); return; }
    const size_t want = std::min<size_t>(n, 8);
    host_parallel(want << 20, [&](int t, int nt) { for (size_t i = n * (size_t)t / (size_t)nt; i < n * (size_t)(t + 1) / (size_t)nt; i++) f(i); });
}

// The chunks as ONE call: every array is [rows][columns][inner] - row r of a chunk goes to row r of the packed array at the chunk's column
// offset (pinned set Q.pinned) - then nomcica_host on the packed arrays, then the outputs back to every chunk.  Caller holds the entry lock.
// d: what the chunks share (nlay, idrv, the cloud flags, permuteseed), icld_in: their icld.  kind 0: rrtmg_lw (non-McICA); kind 1: the
// fused sub-column generator + McICA solver with the kissvec generator (a stream per column: the columns of a packed call draw what they
// draw on their own) and - has_alpha - the generator's alpha array
static int mcica_subcol_host(const CallDesc &d, const GcmIn &g, const double *alpha, const FluxOut &out);
static int solve_chunks(const std::vector<QueuedChunk> &chunks, long long N, CallDesc d, int icld_in, int kind = 0, bool has_alpha = false)
{
    const size_t L = (size_t)d.nlay;
    auto doubles = [&](int a) { return CALL_ARRAYS[a].inner * rows_of(a, L) * (size_t)N; };
    size_t tot = has_alpha ? doubles(A_ALPHA) : 0;
    for (int a = 0; a < NA_GCM; a++) tot += doubles(a);
    for (int a = A_UFLX; a < A_UFLXS; a++) tot += doubles(a);
    if (Q.pinned.bytes() < tot * sizeof(double)) {
        if (Q.pinned) forget_pinned(Q.pinned.get());
        if (int rc = grow(Q.pinned, tot * sizeof(double), tot * sizeof(double), "queue staging")) return rc;
        g_pinned.emplace_back(Q.pinned.as<const char>(), tot * sizeof(double));
    }
    double *in_p[NA_IN] = {}, *out_p[NA_CALL] = {};
    double *p = Q.pinned.as<double>();
    for (int a = 0; a < NA_GCM; a++) { in_p[a] = p; p += doubles(a); }
    for (int a = A_UFLX; a < A_UFLXS; a++) { out_p[a] = p; p += doubles(a); }
    if (has_alpha) in_p[A_ALPHA] = p;
    const bool cloud = !(icld_in == 0);
    std::vector<size_t> offs(chunks.size());
    { size_t off = 0; for (size_t i = 0; i < chunks.size(); i++) { offs[i] = off; off += (size_t)chunks[i].d.ncol; } }
    queue_parallel(chunks.size(), [&](size_t i) {          // (the copies are many short rows: host-bound, spread over a few threads)
        const QueuedChunk &c = chunks[i];
        const double *src[NA_IN];
        gcm_pointers(c.in, c.alpha, src);
        for (int a = 0; a < NA_IN; a++) {
            if (!in_p[a] || (CALL_ARRAYS[a].cloud && !cloud)) continue;
            const size_t inner = CALL_ARRAYS[a].inner, w = inner * (size_t)c.d.ncol;
            for (size_t r = 0; r < rows_of(a, L); r++)
                memcpy(in_p[a] + (r * (size_t)N + offs[i]) * inner, src[a] + r * w, w * sizeof(double));
        }
    });
    int icld = icld_in, irng = 0;
    d.ncol = (int)N; d.icld = &icld; d.irng = &irng;
    FluxOut out = flux_from(out_p);
    if (d.idrv != 1) out.duflx_dt = out.duflxc_dt = nullptr;
    const int rc = kind == 1 ? mcica_subcol_host(d, gcm_from(in_p), in_p[A_ALPHA], out) : nomcica_host(d, gcm_from(in_p), out);
    if (rc == 0) {
        queue_parallel(chunks.size(), [&](size_t i) {
            const QueuedChunk &c = chunks[i];
            double *dst[NA_CALL];
            flux_pointers(c.out, dst);
            for (int a = A_UFLX; a < A_UFLXS; a++) {
                if (!dst[a] || (a >= A_DUFLX_DT && d.idrv != 1)) continue;
                for (size_t r = 0; r < rows_of(a, L); r++)
                    memcpy(dst[a] + r * (size_t)c.d.ncol, out_p[a] + r * (size_t)N + offs[i], (size_t)c.d.ncol * sizeof(double));
            }
            if (c.d.icld) *c.d.icld = icld;
        });
    }
    return rc;
}

extern "C" int rrtmg_lw_hip_queue_flush(void)
{
    ENTRY_LOCK;             // held over pack, solve and scatter: another thread's queue_add / queue_begin / finalize must not touch the chunk list or the pinned set in between
    if (!Q.open) return fail(RRTMG_LW_HIP_EARG, "rrtmg_lw_hip_queue_begin has not been called");
    if (Q.ncol == 0) return 0;
    const int rc = solve_chunks(Q.chunks, Q.ncol, CallDesc{0, Q.nlay, nullptr, Q.idrv, Q.inflg, Q.iceflg, Q.liqflg}, Q.icld);
    Q.chunks.clear();
    Q.ncol = 0;
    return rc;
}

// ---------------------------------------------------------------------------------------------------
// Concurrent callers (threading): a host model that calls rrtmg_lw per chunk of columns from several OpenMP threads.
// The reference is serial inside a call and hosts thread OVER calls (src/rrtmg_lw_rad.nomcica.f90:472); here a call costs ~0.9 ms
// whatever its size below a few thousand columns, so N threads taking turns at one lock run at one chunk per 0.9 ms.  Instead a caller
// that finds another call in flight leaves its request in a list and sleeps; whoever holds the turn solves everything that has gathered
// with the same (nlay, icld, idrv, cloud flags) as ONE packed call (solve_chunks, the queue's own code) and wakes the owners.  Results do
// not depend on the company a chunk had (tests/test_hip_parity.py::test_a_column_does_not_depend_on_its_neighbours).  No call-site change.
// ---------------------------------------------------------------------------------------------------
namespace {
struct CallReq {
    QueuedChunk c;
    int icld = 0;                              // *c.d.icld when the call came in
    int kind = 0;                              // kind 1: the fused generator + McICA entry (kissvec); see solve_chunks
    int rc = 0;
    bool done = false, lead = false;
    std::string err;                           // the text of rc != 0, handed to the owner's thread
    std::condition_variable cv;
};
std::mutex g_comb_mu;
std::condition_variable g_comb_arrive;      // a request has joined the list
std::vector<CallReq *> g_comb_pending;
bool g_comb_busy = false;
size_t g_comb_last = 1;                      // requests the previous pass served: so many callers are about to come back
std::atomic<long long> g_comb_calls{0}, g_comb_passes{0};
// calls of up to this many columns are candidates (larger ones fill the device on their own and go straight to the entry lock)
const int COMBINE_MAX = []() { const char *e = getenv("RRTMG_LW_COMBINE_MAX"); return e ? atoi(e) : 8192; }();
const int COMBINE_WAIT_US = []() { const char *e = getenv("RRTMG_LW_COMBINE_WAIT_US"); return e ? atoi(e) : 250; }();

// everything that has gathered, group by group (the first request's shape, then what is left, ...)
void comb_serve(std::vector<CallReq *> &batch)
{
    ENTRY_LOCK;
    std::vector<char> served(batch.size(), 0);
    for (size_t i = 0; i < batch.size(); i++) {
        if (served[i]) continue;
        CallReq &a = *batch[i];
        std::vector<size_t> grp;
        long long N = 0;
        for (size_t j = i; j < batch.size(); j++) {
            const CallReq &b = *batch[j];
            const CallDesc &x = a.c.d, &y = b.c.d;
            if (!served[j] && y.nlay == x.nlay && b.icld == a.icld && y.idrv == x.idrv && y.inflg == x.inflg && y.iceflg == x.iceflg && y.liqflg == x.liqflg &&
                b.kind == a.kind && y.permuteseed == x.permuteseed && (b.c.alpha != nullptr) == (a.c.alpha != nullptr) &&
                N + y.ncol <= 0x7fffffffLL) { grp.push_back(j); N += y.ncol; }
        }
        auto alone = [&](CallReq &r) {
            int icld = r.icld, irng = 0;
            CallDesc d = r.c.d;
            d.icld = &icld; d.irng = &irng;
            g_comb_passes++;
            r.rc = r.kind == 1 ? mcica_subcol_host(d, r.c.in, r.c.alpha, r.c.out) : nomcica_host(d, r.c.in, r.c.out);
            if (r.c.d.icld) *r.c.d.icld = icld;
            if (r.rc != 0) r.err = G.err;
        };
        if (grp.size() == 1) alone(a);
        else {
            std::vector<QueuedChunk> chunks;
            for (size_t j : grp) chunks.push_back(batch[j]->c);
            g_comb_passes++;
            const int rc = solve_chunks(chunks, N, a.c.d, a.icld, a.kind, a.c.alpha != nullptr);
            if (rc == 0) { for (size_t j : grp) batch[j]->rc = 0; }
            else { for (size_t j : grp) alone(*batch[j]); }      // an error (one caller's bad particle size ...) belongs to the call that caused it: each chunk again, on its own
        }
        for (size_t j : grp) served[j] = 1;
    }
}

int comb_call(CallReq &me)
{
    std::unique_lock<std::mutex> lk(g_comb_mu);
    g_comb_calls++;
    g_comb_pending.push_back(&me);
    g_comb_arrive.notify_one();
    if (g_comb_busy) {
        me.cv.wait(lk, [&] { return me.done || me.lead; });
        if (me.done) { if (me.rc != 0) tl_err = me.err; return me.rc; }
    }
    g_comb_busy = true;                      // this thread has the turn: its own request is among the pending ones
    while (!me.done) {
        // The callers the previous pass served come back within the time of a call's return trip: a pass that starts the moment the first of
        // them is here serves that one alone while the others queue up behind it (measured: passes of 1 and 15 chunks in turn).  Wait for as
        // many as there were, a fraction of a pass's own time at most; a single-threaded host (previous pass: one request) never waits.
        // The window adapts: a wait that ended with everybody here keeps (or restores) it, one that ran out halves it - two threads of
        // which one comes back only after ten milliseconds of its own work must not cost the other 250 us per call - and every 64th pass
        // tries a short window again.
        if (g_comb_last > 1) {
            static int window_us = COMBINE_WAIT_US;
            static unsigned npass = 0;
            int w = window_us;
            if (w < 20 && (++npass & 63u) == 0u) w = std::min(60, COMBINE_WAIT_US);
            if (w >= 20) {
                const bool all = g_comb_arrive.wait_for(lk, std::chrono::microseconds(w), [&] { return g_comb_pending.size() >= g_comb_last; });
                window_us = all ? std::min(COMBINE_WAIT_US, std::max(60, 2 * w)) : w / 2;
            }
        }
        std::vector<CallReq *> batch;
        batch.swap(g_comb_pending);
        g_comb_last = batch.size();
        lk.unlock();
        {   // (the chunks of other callers go through fail() on this thread: their texts are theirs - CallReq::err - not this thread's)
            const std::string mine = tl_err;
            comb_serve(batch);
            tl_err = mine;
        }
        lk.lock();
        for (CallReq *r : batch) { r->done = true; if (r != &me) r->cv.notify_one(); }
    }
    if (!g_comb_pending.empty()) { g_comb_pending.front()->lead = true; g_comb_pending.front()->cv.notify_one(); }     // the turn goes to the first of those who came meanwhile
    else g_comb_busy = false;
    if (me.rc != 0) tl_err = me.err;
    return me.rc;
}

int comb_max() { return COMBINE_MAX; }
bool comb_enabled() { static const bool on = []() { const char *e = getenv("RRTMG_LW_COMBINE"); return !e || atoi(e) != 0; }(); return on; }
long long comb_calls_total() { return g_comb_calls.load(); }
long long comb_passes_total() { return g_comb_passes.load(); }

// what a packed call could not report per chunk is checked per call, before it joins one: null arrays (the packing would read them), nlay
bool packable(const CallDesc &d, const GcmIn &g, const FluxOut &out, bool need_cloud)
{
    if (!have_outs(out) || (d.idrv == 1 && (!out.duflx_dt || !out.duflxc_dt)) || d.nlay < 1 || d.nlay > 603) return false;
    const double *in[NA_IN];
    gcm_pointers(g, nullptr, in);
    for (int a = 0; a < NA_GCM; a++) if (!in[a] && (need_cloud || !CALL_ARRAYS[a].cloud)) return false;
    return true;
}

int nomcica_combined(const CallDesc &d, const GcmIn &g, const FluxOut &out)
{
    const int icld_eff = (*d.icld < 0 || *d.icld > 3) ? 2 : *d.icld;
    if (!packable(d, g, out, icld_eff != 0)) {          // let the plain entry say what is wrong
        ENTRY_LOCK;
        return nomcica_host(d, g, out);
    }
    CallReq me;
    me.c = QueuedChunk{d, g, nullptr, out};
    me.icld = *d.icld;
    return comb_call(me);
}
}   // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------------
// McICA flavour
// ---------------------------------------------------------------------------------------------------
#define MCICA_PARAMS                                                                                            \
    int ncol, int nlay, int *icld, int idrv, GCM_PARAMS, int inflglw, int iceflglw, int liqflglw,               \
    const double *cldfmcl, const double *taucmcl, const double *ciwpmcl, const double *clwpmcl,                 \
    const double *reicmcl, const double *relqmcl, const double *tauaer, OUT_PARAMS

static int mcica_device(const CallDesc &d, const GcmIn &g, const McIn &m, const FluxOut &out, void *stream)
{
    ENTRY_LOCK_FOR(g.play);
    if (int rc = check_mcica_build()) return rc;
    if (int rc = check_call(d, out)) return rc;
    const int mode = *d.icld == 0 ? 0 : 3;                       // inatm leaves the cloud arrays zero when icld = 0 (:899-911)
    const int nbmax = balanced_batch(d.ncol, eff_batch(d.nlay));
    if (int rc = ensure_workspace(d.nlay, nbmax, mode != 0, mode == 3, d.idrv, mode)) return rc;
    return run_pipelined((hipStream_t)stream, batch_of(d, mode, &m), g, out);
}
int rrtmg_lw_hip_run_mcica_device(MCICA_PARAMS, void *stream)
{
    return mcica_device({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}, {GCM_NAMES, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tauaer}, {cldfmcl, taucmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl}, {OUT_NAMES}, stream);
}
int rrtmg_lw_hip_run_mcica_spectral_device(MCICA_PARAMS, SPEC_PARAMS, void *stream)
{
    return mcica_device(spectral({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}), {GCM_NAMES, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tauaer}, {cldfmcl, taucmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl}, {OUT_NAMES, SPEC_NAMES}, stream);
}

static int mcica_host(const CallDesc &d, const GcmIn &g, const McIn &m, const FluxOut &out)
{
    ENTRY_LOCK;
    if (int rc = check_mcica_build()) return rc;
    if (int rc = check_call(d, out)) return rc;
    const int ncol = d.ncol, nlay = d.nlay, idrv = d.idrv;
    const int mode = *d.icld == 0 ? 0 : 3;
    const bool cloud = mode == 3;
    return fan_out(ncol, [&](int c0, int c1) -> int {     // (one block of columns per device of rrtmg_lw_hip_init_devices)
    if (int rc = check_common(ncol, nlay)) return rc;
    HIP_TRY(hipDeviceSynchronize());        // asynchronous device-entry work of earlier calls shares the workspace
    // the sub-column arrays are 4 x 140 x nlay doubles per column: bound the batch so that staging stays below ~4 GB
    const int mcmax = (int)std::max<size_t>(64, ((size_t)1 << 30) / ((size_t)4 * NGPT * nlay * (8 + (d.esz == 4 ? 4 : 0))));        // (HOST_SETS staging sets of 1 GiB; float32 arrays: with their landing area)
    const int nbmax = balanced_batch(c1 - c0, std::min(std::min(eff_batch(nlay), HOST_BATCH), cloud ? mcmax : HOST_BATCH));
    if (int rc = ensure_workspace(nlay, nbmax, cloud, cloud, idrv, mode)) return rc;
    const size_t L = (size_t)nlay;
    std::vector<HostIn> ins;
    if (int rc = host_ins(ins, g, &m, L, cloud, NGPT, NA_GCM, "", d.esz)) return rc;
    std::vector<HostOut> outs = host_outs(out, L, idrv, d.esz);
    auto body = [&](hipStream_t s, int nb, int, std::vector<HostIn> &in, std::vector<HostOut> &out_) -> int {
        GcmIn gd = staged_gcm(in);          // (the sub-column arrays stand in the cloud arrays' places)
        const McIn md{gd.cldfr, gd.taucld, gd.cicewp, gd.cliqwp, gd.reice, gd.reliq};
        gd.cldfr = gd.taucld = gd.cicewp = gd.cliqwp = gd.reice = gd.reliq = nullptr;
        return run_batch<true>(s, staged_batch(d, mode, nb, &md), gd, ColIn{}, staged_flux(out_));
    };
    // layers whose sub-column cloud fractions are all below cldmin for the batch: cldprmc reads nothing else of them (src/rrtmg_lw_cldprmc.f90:182-183)
    std::vector<unsigned char> cloudfree(L, 0), cf_uni(L, 0);
    std::vector<uint64_t> cf_bits(L, 0);
    auto prep = [&](int, int col0, int nb, hipStream_t) -> int {
        if (!cloud) return 0;
        if (d.esz == 4) rows_below((const float *)m.cldfmcl, NGPT, L, (size_t)ncol, (size_t)col0, (size_t)nb, 1.e-20, cloudfree.data(), cf_uni.data(), cf_bits.data());
        else rows_below(m.cldfmcl, NGPT, L, (size_t)ncol, (size_t)col0, (size_t)nb, 1.e-20, cloudfree.data(), cf_uni.data(), cf_bits.data());
        skip_cloudfree(ins, cloudfree.data(), cf_uni.data(), cf_bits.data());
        return 0;
    };
    if (int rc = host_pipeline(ncol, c0, c1, nbmax, ins, outs, body, prep)) return rc;
    hipStream_t s = G.stream.get();
    return read_physics_error(s);
    });
}
int rrtmg_lw_hip_run_mcica(MCICA_PARAMS)
{
    return mcica_host({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}, {GCM_NAMES, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tauaer}, {cldfmcl, taucmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl}, {OUT_NAMES});
}
int rrtmg_lw_hip_run_mcica_r4(int ncol, int nlay, int *icld, int idrv, GCM_PARAMS_R4, int inflglw, int iceflglw, int liqflglw,
    const float *cldfmcl, const float *taucmcl, const float *ciwpmcl, const float *clwpmcl, const float *reicmcl, const float *relqmcl,
    const float *tauaer, OUT_PARAMS_R4)
{
    return mcica_host(real4({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}), {GCM_NAMES_AS, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, AS_(tauaer)},
                      {AS_(cldfmcl), AS_(taucmcl), AS_(ciwpmcl), AS_(clwpmcl), AS_(reicmcl), AS_(relqmcl)}, {OUT_NAMES_AS});
}
int rrtmg_lw_hip_run_mcica_spectral(MCICA_PARAMS, SPEC_PARAMS)
{
    return mcica_host(spectral({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}), {GCM_NAMES, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tauaer}, {cldfmcl, taucmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl}, {OUT_NAMES, SPEC_NAMES});
}

int rrtmg_lw_hip_get_alpha(int ncol, int nlay, int icld, int idcor, double decorr_con, const double *dz, const double *lat,
                           int juldat, const double *cldfrac, double *alpha)
{
    ENTRY_LOCK;
    if (int rc = check_common(ncol, nlay)) return rc;
    if (G.init) HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    if (!(icld == 4 || icld == 5)) return 0;                      // alpha is only defined for the exponential overlaps
    const size_t n = (size_t)ncol, L = (size_t)nlay;
    std::vector<HostIn> ins = {{dz, 1, L, 0}, {lat, 1, 1, 0}, {cldfrac, 1, L, 0}};
    for (auto &a : ins) if (!a.h) return fail(RRTMG_LW_HIP_EARG, "null input array");
    std::vector<HostOut> outs = {{alpha, L, 0, true}};
    if (int rc = stage_alloc(ins, outs, n)) return rc;
    hipStream_t s = G.stream.get();
    if (int rc = stage_in(ins, n, 0, n, s)) return rc;
    const dim3 grid((ncol + BLOCK - 1) / BLOCK, nlay), block(BLOCK);
    hipLaunchKernelGGL(k_alpha, grid, block, 0, s, ncol, nlay, icld, idcor, decorr_con, (const double *)ins[0].d, (const double *)ins[1].d,
                       juldat, (const double *)ins[2].d, outs[0].d);
    return stage_out(outs, n, 0, n, s);
}

int rrtmg_lw_hip_mcica_subcol_device(
    int ncol, int nlay, int icld, int permuteseed, int *irng, const double *play, const double *cldfrac, const double *ciwp,
    const double *clwp, const double *rei, const double *rel, const double *tauc, const double *alpha,
    double *cldfmcl, double *ciwpmcl, double *clwpmcl, double *reicmcl, double *relqmcl, double *taucmcl, void *stream)
{
    ENTRY_LOCK_FOR(play, irng && *irng != 0);
    if (int rc = check_mcica_build()) return rc;
    if (int rc = check_subcol_args(ncol, nlay, icld, irng)) return rc;
    if (icld == 0) return 0;                                      // src/mcica_subcol_gen_lw.f90:265
    hipStream_t s = (hipStream_t)stream;
    if (int rc = generate_mask(s, ncol, nlay, icld, permuteseed, *irng, play, cldfrac, alpha)) return rc;
    const size_t tot = (size_t)NGPT * ncol;
    const dim3 grid((unsigned)((tot + BLOCK - 1) / BLOCK), nlay), block(BLOCK);
    LAUNCH("k_subcol_expand", k_subcol_expand, grid, block, s, G.W, ciwp, clwp, tauc, ncol, nlay, 0, cldfmcl, ciwpmcl, clwpmcl, taucmcl);
    HIP_TRY(hipMemcpyAsync(reicmcl, rei, (size_t)ncol * nlay * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(relqmcl, rel, (size_t)ncol * nlay * 8, hipMemcpyDeviceToDevice, s));
    return 0;
}

// columns [c0, c1) of the stand-alone generator with host arrays (ncol columns wide) on the calling thread's current device state
static int subcol_host_range(
    int ncol, int c0, int c1, int nlay, int icld, int permuteseed, int irng, const double *play, const double *cldfrac, const double *ciwp,
    const double *clwp, const double *rei, const double *rel, const double *tauc, const double *alpha,
    double *cldfmcl, double *ciwpmcl, double *clwpmcl, double *reicmcl, double *relqmcl, double *taucmcl)
{
    HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    const size_t n = (size_t)ncol, L = (size_t)nlay, nl = (size_t)(c1 - c0);
    const bool two = icld == 4 || icld == 5;
    // (only what the generator reads travels: pressures, cloud fractions, alpha; water paths and optical depths stay with the host threads below)
    std::vector<HostIn> ins = {{play, 1, L, 0}, {cldfrac, 1, L, 0}, {two ? alpha : nullptr, 1, L, 0}};
    std::vector<HostOut> outs;                                   // outputs are written by the host threads below
    if (int rc = stage_alloc(ins, outs, nl)) return rc;
    hipStream_t s = G.stream.get();
    if (int rc = stage_in(ins, n, (size_t)c0, nl, s)) return rc;
    if (int rc = generate_mask(s, (int)nl, nlay, icld, permuteseed, irng, ins[0].d, ins[1].d, ins[2].d)) return rc;
    // The sub-column arrays are implied by the mask (MASK_WORDS x 4 B per (column, layer)) and the grid-mean inputs, which the host holds:
    // the mask comes back over PCIe and the host threads write the four (ngpt, ncol, nlay) arrays - 4 x ngpt x 8 B per (column, layer), 224
    // times the mask - at memory speed (src/mcica_subcol_gen_lw.f90:664-680: where cloudy the layer's water paths and the band's optical
    // depth, elsewhere zero).  (Expanding on the device and copying 322 KB per 72-layer column back ran at 0.03 M columns/s.)
    std::vector<unsigned> hmask((size_t)MASK_WORDS * L * nl);
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = bounce_d2h(hmask.data(), G.mask.get(), hmask.size() * sizeof(unsigned))) return rc;
    int gband[NGPT];
    for (int ig = 0; ig < NGPT; ig++) { int b = 1; for (int B = 2; B <= NBND; B++) b += (ig >= band_g0(B)) ? 1 : 0; gband[ig] = b - 1; }
    host_parallel((size_t)NGPT * nl * L * 8 * 4, [&](int t, int nt) {
        const size_t cells = nl * L;
        for (size_t ci = cells * (size_t)t / (size_t)nt; ci < cells * (size_t)(t + 1) / (size_t)nt; ci++) {
            const size_t l = ci / nl, lc = ci % nl;                    // the block's (column, layer) order
            const size_t cl = (size_t)c0 + lc + n * l;                 // ... and the cell's place in the caller's arrays
            unsigned w[MASK_WORDS];
            for (int k = 0; k < MASK_WORDS; k++) w[k] = hmask[((size_t)k * L + l) * nl + lc];
            const double iw = ciwp[cl], lw = clwp[cl];
            const double *tc = tauc + (size_t)NBND * cl;
            double *o0 = cldfmcl + (size_t)NGPT * cl, *o1 = ciwpmcl + (size_t)NGPT * cl, *o2 = clwpmcl + (size_t)NGPT * cl, *o3 = taucmcl + (size_t)NGPT * cl;
            for (int ig = 0; ig < NGPT; ig++) {
                const bool on = (w[ig >> 5] >> (ig & 31)) & 1u;
                o0[ig] = on ? 1.0 : 0.0;
                o1[ig] = on ? iw : 0.0;
                o2[ig] = on ? lw : 0.0;
                o3[ig] = on ? tc[gband[ig]] : 0.0;
            }
        }
    });
    for (size_t l = 0; l < L; l++) {                            // :283-284
        memcpy(reicmcl + c0 + n * l, rei + c0 + n * l, nl * 8);
        memcpy(relqmcl + c0 + n * l, rel + c0 + n * l, nl * 8);
    }
    return read_physics_error(s);
}

int rrtmg_lw_hip_mcica_subcol(
    int ncol, int nlay, int icld, int permuteseed, int *irng, const double *play, const double *cldfrac, const double *ciwp,
    const double *clwp, const double *rei, const double *rel, const double *tauc, const double *alpha,
    double *cldfmcl, double *ciwpmcl, double *clwpmcl, double *reicmcl, double *relqmcl, double *taucmcl)
{
    ENTRY_LOCK;
    if (int rc = check_mcica_build()) return rc;
    if (int rc = check_subcol_args(ncol, nlay, icld, irng)) return rc;
    if (icld == 0) return 0;
    if (!play || !cldfrac || !ciwp || !clwp || !rei || !rel || !tauc) return fail(RRTMG_LW_HIP_EARG, "null input array");
    if ((icld == 4 || icld == 5) && !alpha) return fail(RRTMG_LW_HIP_EARG, "icld = 4/5 needs alpha");
    if (!cldfmcl || !ciwpmcl || !clwpmcl || !reicmcl || !relqmcl || !taucmcl) return fail(RRTMG_LW_HIP_EARG, "null output array");
    const int rng = *irng;
    auto range = [&](int c0, int c1) -> int {
        return subcol_host_range(ncol, c0, c1, nlay, icld, permuteseed, rng, play, cldfrac, ciwp, clwp, rei, rel, tauc, alpha,
                                 cldfmcl, ciwpmcl, clwpmcl, reicmcl, relqmcl, taucmcl);
    };
    if (rng != 0) return range(0, ncol);          // one Mersenne-Twister stream over all columns (:497-503): the first device draws it
    return fan_out(ncol, range);                  // kissvec: a stream per column (:463-474)
}

// Fused generator + solver: mcica_subcol_lw followed by the McICA rrtmg_lw without materialising the (140,ncol,nlay)
// sub-column arrays (they are implied by the mask and the grid-mean cloud properties).  DEVICE pointers.
#define SUBCOL_PARAMS                                                                                                       \
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng, GCM_PARAMS, int inflglw, int iceflglw, int liqflglw, \
    CLOUD_PARAMS, const double *alpha, const double *tauaer, OUT_PARAMS
// what the averaging entries (rrtmg_lw_hip_run_mcica_samples*) ask of nsamp and seedstep, before anything is written
static int check_samples(const CallDesc &d, int nsamp, int seedstep)
{
    if (nsamp < 1) return fail(RRTMG_LW_HIP_EARG, "nsamp = %d: at least one sample", nsamp);
    if (nsamp > RRTMG_LW_HIP_MAX_SAMPLES) return fail(RRTMG_LW_HIP_EARG, "nsamp = %d exceeds RRTMG_LW_HIP_MAX_SAMPLES = %d", nsamp, RRTMG_LW_HIP_MAX_SAMPLES);
    if (seedstep < 1) return fail(RRTMG_LW_HIP_EARG, "seedstep = %d: the seeds of two samples must differ (at least 1; the sub-columns of a sample, rrtmg_lw_hip_gpoints(), is the documented choice)", seedstep);
    if ((long long)d.permuteseed + (long long)(nsamp - 1) * seedstep > 2147483647ll)
        return fail(RRTMG_LW_HIP_EARG, "permuteseed + (nsamp - 1) * seedstep = %d + %d * %d is not an int", d.permuteseed, nsamp - 1, seedstep);
    if (nsamp > 1 && d.irng && *d.irng != 0) return fail(RRTMG_LW_HIP_EARG, "irng = %d with nsamp = %d: several samples are drawn with the kissvec generator (irng = 0) only", *d.irng, nsamp);
    return 0;
}
// ... and of the optional variance arrays: a variance needs two samples, and M of the recurrence cannot live where S does.  level_bytes,
// layer_bytes: what a (., nlay+1) and a (., nlay) array span from their pointers in the caller's form.
static int check_var(const FluxOut &o, int nsamp, size_t level_bytes, size_t layer_bytes)
{
    const struct { const double *v, *m; size_t n; const char *name; } t[3] = {{o.uflx_var, o.uflx, level_bytes, "uflx"}, {o.dflx_var, o.dflx, level_bytes, "dflx"}, {o.hr_var, o.hr, layer_bytes, "hr"}};
    for (const auto &e : t) {
        if (!e.v) continue;
        if (nsamp == 1) return fail(RRTMG_LW_HIP_EARG, "%s_var with nsamp = 1: the sample variance needs at least two samples (pass NULL)", e.name);
        const char *v = (const char *)e.v, *m = (const char *)e.m;
        const size_t n = e.n;
        if (m && v < m + n && m < v + n) return fail(RRTMG_LW_HIP_EARG, "%s_var aliases %s: the two sums of a sample are kept in the two arrays", e.name, e.name);
    }
    return 0;
}
static FluxOut with_var(FluxOut o, double *uflx_var, double *dflx_var, double *hr_var)
{
    o.uflx_var = uflx_var; o.dflx_var = dflx_var; o.hr_var = hr_var;
    return o;
}
// the fused call on stream s (the caller holds the lock): the checks, the workspace, the mask buffer, then run_pipelined - or, with
// nsamp > 1 and cloud, run_samples: the seeds permuteseed + i seedstep batch by batch and sample by sample on that one stream, the gas
// optics of a batch once (the workspace is then that of the McICA entry with sub-column arrays: W.odg holds the float64 optical depths)
static int mcica_subcol_device_run(const CallDesc &d, const GcmIn &g, const double *alpha, const FluxOut &out, hipStream_t s, int nsamp = 1, int seedstep = 1)
{
    if (int rc = check_mcica_build()) return rc;
    if (d.spectral) if (int rc = check_spec(out)) return rc;
    if (!d.icld) return fail(RRTMG_LW_HIP_EARG, "icld is null");
    if (int rc = check_subcol_args(d.ncol, d.nlay, *d.icld, d.irng)) return rc;
    if (d.idrv == 1 && (!out.duflx_dt || !out.duflxc_dt)) return fail(RRTMG_LW_HIP_EARG, "idrv=1 needs duflx_dt and duflxc_dt");
    const int icld_gen = *d.icld;
    if (*d.icld > 3) *d.icld = 2;                                 // what rrtmg_lw does to the generator's icld (src/rrtmg_lw_rad.f90:469)
    const int mode = icld_gen == 0 ? 0 : 3;
    const int nbmax = balanced_batch(d.ncol, eff_batch(d.nlay));
    // mask path: no per-g-point cloud arrays - but for the float64 optical depths the samples of an averaging call share (W.odg)
    if (int rc = ensure_workspace(d.nlay, nbmax, mode != 0, mode == 3 && nsamp > 1, d.idrv, mode)) return rc;
    KissGen gen{false, icld_gen, d.permuteseed, alpha};
    if (mode == 3) {
        if (*d.irng == 0) {          // kissvec: every column owns its stream -> generated batch by batch on the auxiliary stream
            if (int rc = prepare_mask(d.ncol, d.nlay, icld_gen, 0, alpha)) return rc;
            gen.on = true;
        } else {
            // the Mersenne-Twister stream runs over the ncol columns of the call, in call order, and its kernels take arrays as wide as
            // the call: a *_view call with a wider ld stages play, cldfr and alpha call-wide first, as the *_as entry does
            const double *gp = g.play, *gc = g.cldfr, *ga = alpha;
            if (d.ld > 0 && d.ld != d.ncol) { if (int rc = stage_generator_arrays(s, d, icld_gen, &gp, &gc, &ga)) return rc; }
            if (int rc = generate_mask(s, d.ncol, d.nlay, icld_gen, d.permuteseed, *d.irng, gp, gc, ga)) return rc;
        }
    }
    if (mode != 3 || nsamp == 1) return run_pipelined(s, batch_of(d, mode), g, out, gen);          // (no cloud: nothing is drawn, every sample is the same)
    return run_samples(s, batch_of(d, mode), g, out, gen, nsamp, seedstep);
}
static int mcica_subcol_device(const CallDesc &d, const GcmIn &g, const double *alpha, const FluxOut &out, void *stream)
{
    ENTRY_LOCK_FOR(g.play, d.irng && *d.irng != 0);
    return mcica_subcol_device_run(d, g, alpha, out, (hipStream_t)stream);
}
#define SAMPLES_PARAMS                                                                                                                        \
    int ncol, int nlay, int *icld, int idrv, int permuteseed, int nsamp, int seedstep, int *irng, GCM_PARAMS, int inflglw, int iceflglw, int liqflglw, \
    CLOUD_PARAMS, const double *alpha, const double *tauaer, OUT_PARAMS
int rrtmg_lw_hip_run_mcica_samples_device(SAMPLES_PARAMS, void *stream)
{
    const CallDesc d{ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng};
    ENTRY_LOCK_FOR(play, irng && *irng != 0);
    if (int rc = check_samples(d, nsamp, seedstep)) return rc;
    return mcica_subcol_device_run(d, {GCM_NAMES, CLOUD_NAMES, tauaer}, alpha, {OUT_NAMES}, (hipStream_t)stream, nsamp, seedstep);
}
int rrtmg_lw_hip_run_mcica_subcol_device(SUBCOL_PARAMS, void *stream)
{
    return mcica_subcol_device({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng}, {GCM_NAMES, CLOUD_NAMES, tauaer}, alpha, {OUT_NAMES}, stream);
}
int rrtmg_lw_hip_run_mcica_subcol_spectral_device(SUBCOL_PARAMS, SPEC_PARAMS, void *stream)
{
    return mcica_subcol_device(spectral({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng}), {GCM_NAMES, CLOUD_NAMES, tauaer}, alpha, {OUT_NAMES, SPEC_NAMES}, stream);
}

// columns [c0, c1) of the fused generator + solver call on the calling thread's current device state (kissvec seeds its stream per
// column, src/mcica_subcol_gen_lw.f90:463-474: a block of columns is generated and solved on its own; the Mersenne-Twister stream is one
// sequence over all columns of a call, :497-503, and is drawn with c0 = 0, c1 = ncol only)
static int mcica_subcol_host_range(const CallDesc &d, int icld_gen, int irng, int c0, int c1, const GcmIn &g, const double *alpha, const FluxOut &out)
{
    const int ncol = d.ncol, nlay = d.nlay, idrv = d.idrv;
    if (int rc = check_common(ncol, nlay)) return rc;
    HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    const int mode = icld_gen == 0 ? 0 : 3;
    const bool cloud = mode == 3, two = icld_gen == 4 || icld_gen == 5;
    const int nloc = c1 - c0;
    const int nbmax = balanced_batch(nloc, std::min(eff_batch(nlay), HOST_BATCH));
    if (int rc = ensure_workspace(nlay, nbmax, cloud, false, idrv, mode)) return rc;
    const size_t L = (size_t)nlay, n = (size_t)ncol, nl = (size_t)nloc;
    hipStream_t s = G.stream.get();
    // 1. masks of the block's columns: needs play, cldfr, alpha of every one of them
    if (cloud) {
        if (!g.play || !g.cldfr || (two && !alpha)) return fail(RRTMG_LW_HIP_EARG, "null generator input");
        const bool r4 = d.esz == 4;
        DevBuf gen_buf;             // (released when this block is left, on every path)
        if (int rc = grow(gen_buf, nl * L * (r4 ? 12 : 8) * 3, nl * L * (r4 ? 12 : 8) * 3, "generator inputs")) return rc;
        double *const d_gen = gen_buf.as<double>();
        // (through the library's own pinned buffer: see bounce_h2d)
        if (r4) {
            // float arrays: the three travel as float32 behind the float64 ones and are widened there (k_widen_rows, an entry each)
            float *f_gen = reinterpret_cast<float *>(d_gen + 3 * nl * L);
            const double *src[3] = {g.play, g.cldfr, two ? alpha : nullptr};
            auto &hs = G.hset[0];
            if (int rc = ensure_hostbuf(hs.widen, 3 * sizeof(RowCvt))) return rc;
            RowCvt *wtab = hs.widen.as<RowCvt>();
            unsigned nw = 0;
            for (size_t a = 0; a < 3; a++) {
                if (!src[a]) continue;
                if (int rc = bounce_h2d_rows(f_gen + a * nl * L, (const float *)src[a] + c0, nl * 4, n * 4, L)) return rc;
                wtab[nw++] = RowCvt{d_gen + a * nl * L, f_gen + a * nl * L, nl * L};
            }
            LAUNCH("k_widen_rows", k_widen_rows, dim3(cvt_blocks(nl * L), nw), dim3(256), s, (const RowCvt *)wtab);
        } else {
            if (int rc = bounce_h2d_rows(d_gen, g.play + c0, nl * 8, n * 8, L)) return rc;
            if (int rc = bounce_h2d_rows(d_gen + nl * L, g.cldfr + c0, nl * 8, n * 8, L)) return rc;
            if (two) { if (int rc = bounce_h2d_rows(d_gen + 2 * nl * L, alpha + c0, nl * 8, n * 8, L)) return rc; }
        }
        if (int rc = generate_mask(s, nloc, nlay, icld_gen, d.permuteseed, irng, d_gen, d_gen + nl * L, two ? d_gen + 2 * nl * L : nullptr)) return rc;
        if (hipStreamSynchronize(s) != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "generator failed");      // (the generator has read d_gen before it goes)
    }
    // 2. column batches
    std::vector<HostIn> ins;
    if (int rc = host_ins(ins, g, nullptr, L, cloud, NBND, NA_GCM, "", d.esz)) return rc;
    if (!have_outs(out)) return fail(RRTMG_LW_HIP_EARG, "null output array");
    std::vector<HostOut> outs = host_outs(out, L, idrv, d.esz);
    auto body = [&](hipStream_t bs, int nb, int col0, std::vector<HostIn> &in, std::vector<HostOut> &out_) -> int {
        G.W.mask_col0 = (size_t)(col0 - c0);                      // staged arrays start at column 0, the mask holds the block's columns
        return run_batch<true>(bs, staged_batch(d, mode, nb), staged_gcm(in), ColIn{}, staged_flux(out_));
    };
    {
        const int rc = host_pipeline(ncol, c0, c1, nbmax, ins, outs, body);
        if (rc) { G.W.mask_col0 = 0; return rc; }
    }
    G.W.mask_col0 = 0;
    return read_physics_error(s);
}

}   // extern "C"
// the fused entry behind the lock (the caller holds it): argument checks, the columns over the devices
static int mcica_subcol_host(const CallDesc &d, const GcmIn &g, const double *alpha, const FluxOut &out)
{
    if (int rc = check_mcica_build()) return rc;
    if (d.spectral) if (int rc = check_spec(out)) return rc;
    if (!d.icld) return fail(RRTMG_LW_HIP_EARG, "icld is null");
    if (int rc = check_subcol_args(d.ncol, d.nlay, *d.icld, d.irng)) return rc;
    if (d.idrv == 1 && (!out.duflx_dt || !out.duflxc_dt)) return fail(RRTMG_LW_HIP_EARG, "idrv=1 needs duflx_dt and duflxc_dt");
    const int icld_gen = *d.icld, rng = *d.irng;
    if (*d.icld > 3) *d.icld = 2;
    auto range = [&](int c0, int c1) -> int { return mcica_subcol_host_range(d, icld_gen, rng, c0, c1, g, alpha, out); };
    // the Mersenne-Twister stream (irng = 1) is ONE sequence over the (sub-column, column, layer) draws of the call
    // (src/mcica_subcol_gen_lw.f90:497-503): a column's deviates depend on every column before it, so the call stays on the first device
    if (rng != 0 && icld_gen != 0) return range(0, d.ncol);
    return fan_out(d.ncol, range);
}
extern "C" {
int rrtmg_lw_hip_run_mcica_subcol(SUBCOL_PARAMS)
{
    const CallDesc d{ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng};
    const GcmIn g{GCM_NAMES, CLOUD_NAMES, tauaer};
    const FluxOut out{OUT_NAMES};
    // a small call with the kissvec generator (every column draws from its own stream: src/mcica_subcol_gen_lw.f90:463-474) that finds
    // another in flight is solved together with it in one pass, like the non-McICA entry (comb_call); the Mersenne Twister - one stream
    // over the columns of a call - and calls that are wrong on their face take the lock and say so themselves
    const bool plain = ncol >= 1 && ncol <= comb_max() && comb_enabled() && icld && irng && *irng == 0 && *icld >= 0 && *icld <= 5 && packable(d, g, out, true);
    if (plain) {
        CallReq me;
        me.c = QueuedChunk{d, g, alpha, out};
        me.icld = *icld;
        me.kind = 1;
        return comb_call(me);
    }
    ENTRY_LOCK;
    return mcica_subcol_host(d, g, alpha, out);
}

}   // extern "C"
// The mean over nsamp samples from HOST arrays (the entry lock, the first device, no combining).  The samples add up in the output
// arrays on the device (k_flux_acc), so the call's arrays live there as a whole for its duration - not batch by batch in the staging
// sets as the single call's do -, the device path runs on them, and the outputs travel back once.
// (out.uflx_var, dflx_var, hr_var: rrtmg_lw_hip_run_mcica_samples_var - three more arrays of the per-call allocation; with *icld = 0 the
// call then takes this path too: sample 0's k_flux writes their zeros)
static int samples_host(const CallDesc &d, const GcmIn &g, const double *alpha, const FluxOut &out, int nsamp, int seedstep)
{
    const int ncol = d.ncol, nlay = d.nlay, idrv = d.idrv;
    int *const icld = d.icld, *const irng = d.irng;
    double *const duflx_dt = out.duflx_dt, *const duflxc_dt = out.duflxc_dt;
    ENTRY_LOCK;
    if (int rc = check_samples(d, nsamp, seedstep)) return rc;
    {
        const size_t n8 = (size_t)std::max(ncol, 0) * 8, L0 = (size_t)std::max(nlay, 0);
        if (int rc = check_var(out, nsamp, (L0 + 1) * n8, L0 * n8)) return rc;
    }
    double *const hvar[3] = {out.uflx_var, out.dflx_var, out.hr_var};
    const bool var = hvar[0] || hvar[1] || hvar[2];
    if (nsamp == 1 || !icld || !irng || *icld < (var ? 0 : 1) || *icld > 5) return mcica_subcol_host(d, g, alpha, out);      // (a single sample; no cloud: nothing is drawn; what the single call refuses)
    const bool cloud = *icld != 0;
    if (int rc = check_mcica_build()) return rc;
    if (int rc = check_subcol_args(ncol, nlay, *icld, irng)) return rc;
    if (idrv == 1 && (!duflx_dt || !duflxc_dt)) return fail(RRTMG_LW_HIP_EARG, "idrv=1 needs duflx_dt and duflxc_dt");
    if (!have_outs(out)) return fail(RRTMG_LW_HIP_EARG, "null output array");
    if (cloud && nlay < 4) return fail(RRTMG_LW_HIP_EARG, "the kissvec generator needs at least four layers");
    const bool two = *icld == 4 || *icld == 5;
    if (two && !alpha) return fail(RRTMG_LW_HIP_EARG, "icld = 4/5 needs alpha");
    const double *hin[NA_IN];
    gcm_pointers(g, two ? alpha : nullptr, hin);
    for (int a = 0; a < NA_GCM; a++) {
        if (CALL_ARRAYS[a].cloud && !cloud) hin[a] = nullptr;            // (inatm does not read them: they do not travel)
        else if (!hin[a]) return fail(RRTMG_LW_HIP_EARG, CALL_ARRAYS[a].cloud ? "null cloud array" : "null input array (argument %d)", a);
    }
    double *hout[NA_CALL];
    flux_pointers(out, hout);
    const size_t L = (size_t)nlay, n = (size_t)ncol;
    const auto count = [&](int a) { return CALL_ARRAYS[a].inner * rows_of(a, L) * n; };
    const auto travels = [&](int a) { return a < NA_IN ? hin[a] != nullptr : a < A_DUFLX_DT || idrv == 1; };
    size_t total = 0;
    for (int a = 0; a < A_UFLXS; a++) if (travels(a)) total += count(a);
    const int var_of[3] = {A_UFLX, A_DFLX, A_HR};       // a variance has its mean's shape
    for (int k = 0; k < 3; k++) if (hvar[k]) total += count(var_of[k]);
    HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    DevBuf buf;                             // (released when the call is left, on every path)
    if (int rc = grow(buf, total * 8, total * 8, "arrays of an averaging call")) return rc;
    const double *din[NA_IN] = {};
    double *dout[NA_CALL] = {}, *dvar[3] = {};
    {
        double *p = buf.as<double>();
        for (int a = 0; a < A_UFLXS; a++) {
            if (!travels(a)) continue;
            if (a < NA_IN) { if (int rc = bounce_h2d(p, hin[a], count(a) * 8)) return rc; din[a] = p; }
            else dout[a] = p;
            p += count(a);
        }
        for (int k = 0; k < 3; k++) if (hvar[k]) { dvar[k] = p; p += count(var_of[k]); }
    }
    hipStream_t s = G.stream.get();
    if (int rc = mcica_subcol_device_run(d, gcm_from(din), din[A_ALPHA], with_var(flux_from(dout), dvar[0], dvar[1], dvar[2]), s, nsamp, seedstep)) return rc;
    if (int rc = read_physics_error(s)) return rc;
    for (int a = A_UFLX; a < A_UFLXS; a++) if (dout[a] && hout[a]) { if (int rc = bounce_d2h(hout[a], dout[a], count(a) * 8)) return rc; }
    for (int k = 0; k < 3; k++) if (hvar[k]) { if (int rc = bounce_d2h(hvar[k], dvar[k], count(var_of[k]) * 8)) return rc; }
    return 0;
}
extern "C" {
int rrtmg_lw_hip_run_mcica_samples(SAMPLES_PARAMS)
{
    return samples_host({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng}, {GCM_NAMES, CLOUD_NAMES, tauaer}, alpha, {OUT_NAMES}, nsamp, seedstep);
}
// ... with the unbiased sample variances of uflx, dflx and hr (each optional), formed where the mean is (k_flux_var)
int rrtmg_lw_hip_run_mcica_samples_var(SAMPLES_PARAMS, double *uflx_var, double *dflx_var, double *hr_var)
{
    return samples_host({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng}, {GCM_NAMES, CLOUD_NAMES, tauaer}, alpha,
                        with_var({OUT_NAMES}, uflx_var, dflx_var, hr_var), nsamp, seedstep);
}

// float32 host arrays, alpha too: the entry lock, no combining (like the spectral entry)
int rrtmg_lw_hip_run_mcica_subcol_r4(int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng, GCM_PARAMS_R4, int inflglw, int iceflglw, int liqflglw,
    CLOUD_PARAMS_R4, const float *alpha, const float *tauaer, OUT_PARAMS_R4)
{
    ENTRY_LOCK;
    return mcica_subcol_host(real4({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng}), {GCM_NAMES_AS, CLOUD_NAMES_AS, AS_(tauaer)}, AS_(alpha), {OUT_NAMES_AS});
}

// the same with spectral outputs: does not join the combining entry (the entry lock, like any other call)
int rrtmg_lw_hip_run_mcica_subcol_spectral(SUBCOL_PARAMS, SPEC_PARAMS)
{
    ENTRY_LOCK;
    return mcica_subcol_host(spectral({ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng}), {GCM_NAMES, CLOUD_NAMES, tauaer}, alpha, {OUT_NAMES, SPEC_NAMES});
}

}  // extern "C"

// ---- device arrays in the caller's own form (rrtmg_lw_hip_*_as) ------------------------------------------------------------------------
// The shape of the host-pointer entries (nomcica_host_range, mcica_subcol_host_range, gas_optics_host_range) with kernels where those have
// copies: per batch of columns, on the caller's stream, k_form_in brings the caller's arrays into staged float64 reference-form arrays nb
// columns wide, the solver runs on those (run_batch<true> / run_optics<true>, column 0 of nb), k_form_out takes the staged outputs back.
// Below the entries the caller's arrays travel in GcmIn / FluxOut / OptOut like everywhere else - as addresses only: what they point to
// has the form's element type and layout, and nothing but the two kernels reads or writes through them.
namespace {

struct FormItem { const void *user; int pos; int V, inner, kind; bool vertical; };
// an array of the call by its position (CALL_ARRAYS): the vertical extent, the trailing index of the column-slowest form
FormItem form_item(const void *user, int a, size_t L, int kind = FA_PLANE)
{
    const ArrayShape &sh = CALL_ARRAYS[a];
    if (sh.per_layer == 0) return FormItem{user, a, (int)sh.extra, 1, kind, false};                       // tsfc, emis: no vertical axis
    if (sh.per_layer == 16) return FormItem{user, a, (int)(L + sh.extra / 16), 16, kind, true};          // tauaer
    return FormItem{user, a, (int)(L + sh.extra), kind == FA_PLANE ? 1 : NBND, kind, true};
}
size_t form_doubles(const FormItem &it, size_t nb)
{
    return nb * (size_t)it.V * (size_t)(it.kind == FA_TAUCTOT ? 1 : it.inner);
}
size_t form_tiles(const FormItem &it, size_t nb)
{
    const size_t nct = (nb + FORM_TILE - 1) / FORM_TILE;
    if (it.kind == FA_TAUCLD) return nct * (size_t)it.V;
    const size_t R = (size_t)it.V * (size_t)(it.kind == FA_TAUCTOT ? 1 : it.inner);
    return nct * ((R + FORM_TILE - 1) / FORM_TILE);
}
// staged arrays of the items, packed from `base` for a batch nb columns wide (arrays whose size is a multiple of 16 values first: the rows
// of taucld stay 128-byte aligned); staged[item] = its place.  Returns the doubles used.
size_t form_place(const std::vector<FormItem> &items, size_t nb, double *base, std::vector<double *> &staged)
{
    staged.assign(items.size(), nullptr);
    size_t off = 0;
    for (int pass = 0; pass < 2; pass++)
        for (size_t k = 0; k < items.size(); k++) {
            const bool wide = items[k].kind == FA_TAUCLD || (items[k].kind == FA_PLANE && items[k].inner == 16);
            if (wide != (pass == 0)) continue;
            staged[k] = base ? base + off : nullptr;
            off += form_doubles(items[k], nb);
        }
    return off;
}
// one launch of k_form_in (in = true) or k_form_out over the items; ncol: the columns between two rows of the caller's column-fastest
// arrays (the call's columns, or a *_view call's ld), col0: the batch's first column
int form_launch(hipStream_t s, bool in, const rrtmg_lw_hip_array_form &f, const std::vector<FormItem> &items, const std::vector<double *> &staged,
                size_t ncol, size_t col0, size_t nb)
{
    if (items.empty()) return 0;
    if (items.size() > (size_t)FORM_MAX) return fail(RRTMG_LW_HIP_EARG, "internal: %d arrays in one conversion table", (int)items.size());
    FormTable t{};
    size_t tiles = 0;
    for (size_t k = 0; k < items.size(); k++) {
        FormArray &e = t.a[k];
        e.user = const_cast<void *>(items[k].user);
        e.staged = staged[k];
        e.V = items[k].V; e.inner = items[k].inner; e.kind = items[k].kind;
        e.flip = items[k].vertical && f.top_first ? 1 : 0;
        e.tile0 = (unsigned)tiles;
        tiles += form_tiles(items[k], nb);
    }
    if (tiles > 0x7fffffffull) return fail(RRTMG_LW_HIP_EARG, "internal: conversion grid of %zu workgroups", tiles);
    t.n = (int)items.size(); t.nb = (int)nb; t.layer_fastest = f.layer_fastest; t.ncol = ncol; t.col0 = col0;
    const dim3 grid((unsigned)tiles), block(256);
    if (in) {
        if (f.real_bytes == 4) LAUNCH("k_form_in<f32>", (k_form_in<float>), grid, block, s, t);
        else LAUNCH("k_form_in<f64>", (k_form_in<double>), grid, block, s, t);
    } else {
        if (f.real_bytes == 4) LAUNCH("k_form_out<f32>", (k_form_out<float>), grid, block, s, t);
        else LAUNCH("k_form_out<f64>", (k_form_out<double>), grid, block, s, t);
    }
    return launches_ok();
}
// the staging of a batch / of the generator's call-wide arrays: grows like the workspace, freed by finalize and by a re-initialisation
int ensure_form(DevBuf &b, size_t bytes) { return grow(b, bytes, bytes, "array-form staging"); }

// what the three entries check first; 1 = the plain form (the entry forwards)
int form_check(const rrtmg_lw_hip_array_form *f, bool *plain)
{
    const char *bad = !f ? "array form is null"
                    : (f->real_bytes != 4 && f->real_bytes != 8) ? "array form: real_bytes must be 4 or 8"
                    : (f->layer_fastest != 0 && f->layer_fastest != 1) ? "array form: layer_fastest must be 0 or 1"
                    : (f->top_first != 0 && f->top_first != 1) ? "array form: top_first must be 0 or 1" : nullptr;
    if (bad) { ENTRY_LOCK; return fail(RRTMG_LW_HIP_EARG, "%s", bad); }
    *plain = f->real_bytes == 8 && !f->layer_fastest && !f->top_first;
    return 0;
}

// The batches of a solver call (non-McICA: mode 0 - 2; fused McICA: mode 0 or 3 with the masks of the whole call in G.mask) on stream s.
// u / uo: the caller's arrays.  Caller holds the entry lock, the workspace stands.
int form_solve(const rrtmg_lw_hip_array_form &f, const CallDesc &d, int mode, const GcmIn &u, const FluxOut &uo, hipStream_t s)
{
    const size_t L = (size_t)d.nlay, ncol = (size_t)d.ncol, ldu = d.ld > 0 ? (size_t)d.ld : ncol;
    const bool cloud = mode != 0;
    // with inflglw >= 1 cldprop reads taucld only through its band sum (nomcica_host_range): one staged value per cell instead of sixteen
    const bool use_tot = cloud && mode != 3 && d.inflg != 0;
    const double *up[NA_IN];
    gcm_pointers(u, nullptr, up);
    std::vector<FormItem> ins, outs;
    for (int a = 0; a < NA_GCM; a++) {
        if (CALL_ARRAYS[a].cloud && !cloud) continue;
        if (!up[a]) return fail(RRTMG_LW_HIP_EARG, "null input array (argument %d of rrtmg_lw's arrays)", a + 1);
        ins.push_back(form_item(up[a], a, L, a == A_TAUCLD ? (use_tot ? FA_TAUCTOT : FA_TAUCLD) : FA_PLANE));
    }
    if (!have_outs(uo)) return fail(RRTMG_LW_HIP_EARG, "null output array");
    double *uop[NA_CALL];
    flux_pointers(uo, uop);
    for (int a = A_UFLX; a < A_UFLXS; a++) if (a < A_DUFLX_DT || d.idrv == 1) outs.push_back(form_item(uop[a], a, L));
    // the spectral outputs of a *_view call ((., nlay+1, 16) like planklev): staged only when they are asked for
    for (int a = A_UFLXS; a < NA_CALL; a++) if (uop[a]) outs.push_back(form_item(uop[a], a, L));
    const size_t nbmax = (size_t)balanced_batch(d.ncol, eff_batch(d.nlay));
    std::vector<double *> si, so;
    const size_t n_in = form_place(ins, nbmax, nullptr, si), n_out = form_place(outs, nbmax, nullptr, so);
    if (int rc = ensure_form(G.form_buf, (n_in + n_out) * 8)) return rc;
    if (int rc = ensure_pipeline()) return rc;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the workspace and the staging
    int rc = 0;
    for (size_t col0 = 0; col0 < ncol && rc == 0; col0 += nbmax) {
        const size_t nb = std::min(nbmax, ncol - col0);
        const size_t used = form_place(ins, nb, G.form_buf.as<double>(), si);
        form_place(outs, nb, G.form_buf.as<double>() + used, so);
        const double *sp[NA_IN] = {};
        for (size_t k = 0; k < ins.size(); k++) sp[ins[k].pos] = si[k];
        GcmIn g = gcm_from(sp);
        if (use_tot) { g.tauctot = g.taucld; g.taucld = nullptr; }
        double *op[NA_CALL] = {};
        for (size_t k = 0; k < outs.size(); k++) op[outs[k].pos] = so[k];
        rc = form_launch(s, true, f, ins, si, ldu, col0, nb);
        G.W.mask_col0 = mode == 3 ? col0 : 0;             // staged arrays start at column 0, the mask holds the call's columns
        if (rc == 0) rc = run_batch<true>(s, staged_batch(d, mode, (int)nb), g, ColIn{}, flux_from(op));
        if (rc == 0) rc = form_launch(s, false, f, outs, so, ldu, col0, nb);
    }
    G.W.mask_col0 = 0;
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return rc;
}

int nomcica_device_as(const rrtmg_lw_hip_array_form &f, const CallDesc &d, const GcmIn &u, const FluxOut &uo, void *stream)
{
    ENTRY_LOCK_FOR(u.play);
    if (int rc = check_call(d, uo)) return rc;
    const int mode = *d.icld == 0 ? 0 : (*d.icld == 1 ? 1 : 2);
    const int nbmax = balanced_batch(d.ncol, eff_batch(d.nlay));
    if (int rc = ensure_workspace(d.nlay, nbmax, mode != 0, false, d.idrv, mode)) return rc;
    return form_solve(f, d, mode, u, uo, (hipStream_t)stream);
}

// fused generator + solver (mcica_subcol_host_range): the masks of the whole call first - from play, cldfr and alpha of every column,
// staged call-wide - then the batches
int mcica_subcol_device_as(const rrtmg_lw_hip_array_form &f, const CallDesc &d, const GcmIn &u, const void *alpha, const FluxOut &uo, void *stream)
{
    ENTRY_LOCK_FOR(u.play, d.irng && *d.irng != 0);
    if (int rc = check_mcica_build()) return rc;
    if (d.spectral) if (int rc = check_spec(uo)) return rc;
    if (!d.icld) return fail(RRTMG_LW_HIP_EARG, "icld is null");
    if (int rc = check_subcol_args(d.ncol, d.nlay, *d.icld, d.irng)) return rc;
    if (d.idrv == 1 && (!uo.duflx_dt || !uo.duflxc_dt)) return fail(RRTMG_LW_HIP_EARG, "idrv=1 needs duflx_dt and duflxc_dt");
    const int icld_gen = *d.icld;
    if (*d.icld > 3) *d.icld = 2;                                 // what rrtmg_lw does to the generator's icld (src/rrtmg_lw_rad.f90:469)
    const int mode = icld_gen == 0 ? 0 : 3;
    const bool two = icld_gen == 4 || icld_gen == 5;
    const hipStream_t s = (hipStream_t)stream;
    const int nbmax = balanced_batch(d.ncol, eff_batch(d.nlay));
    if (int rc = ensure_workspace(d.nlay, nbmax, mode != 0, false, d.idrv, mode)) return rc;
    if (mode == 3) {
        if (!u.play || !u.cldfr || (two && !alpha)) return fail(RRTMG_LW_HIP_EARG, two && !alpha ? "icld = 4/5 needs alpha" : "null generator input");
        const size_t L = (size_t)d.nlay, n = (size_t)d.ncol;
        std::vector<FormItem> gen = {form_item(u.play, A_PLAY, L), form_item(u.cldfr, A_CLDFR, L)};
        if (two) gen.push_back(form_item(alpha, A_ALPHA, L));
        std::vector<double *> sg;
        const size_t need = form_place(gen, n, nullptr, sg);
        if (int rc = ensure_form(G.form_gen, need * 8)) return rc;
        form_place(gen, n, G.form_gen.as<double>(), sg);
        if (int rc = ensure_pipeline()) return rc;
        if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));
        if (int rc = form_launch(s, true, f, gen, sg, d.ld > 0 ? (size_t)d.ld : n, 0, n)) return rc;
        if (int rc = generate_mask(s, d.ncol, d.nlay, icld_gen, d.permuteseed, *d.irng, sg[0], sg[1], two ? sg[2] : nullptr)) return rc;
    }
    return form_solve(f, d, mode, u, uo, s);
}

// The sample-aware sibling of form_solve (rrtmg_lw_hip_run_mcica_samples_device_view with a converting form, nsamp > 1: the kissvec
// generator).  Per batch the caller's arrays - alpha too - are staged ONCE, the samples run on the staged arrays as run_samples runs
// them on a caller's (the sums live in the staged output planes, the variance planes beside them), and the outputs are converted once,
// after the last sample: a float32 output is rounded once.  The generator draws per staged batch, at column 0 of the staged arrays
// and of the mask (Workspace::mask_col0 = 0); the whole-call mask of mcica_subcol_device_as holds ONE sample and is not used.
// Caller holds the entry lock.
int mcica_samples_as_run(const rrtmg_lw_hip_array_form &f, const CallDesc &d, const GcmIn &u, const void *alpha, const FluxOut &uo, int nsamp, int seedstep, hipStream_t s)
{
    if (int rc = check_mcica_build()) return rc;
    if (!d.icld) return fail(RRTMG_LW_HIP_EARG, "icld is null");
    if (int rc = check_subcol_args(d.ncol, d.nlay, *d.icld, d.irng)) return rc;
    if (d.idrv == 1 && (!uo.duflx_dt || !uo.duflxc_dt)) return fail(RRTMG_LW_HIP_EARG, "idrv=1 needs duflx_dt and duflxc_dt");
    const int icld_gen = *d.icld;
    const int mode = icld_gen == 0 ? 0 : 3;
    const bool cloud = mode != 0, two = icld_gen == 4 || icld_gen == 5;
    const size_t L = (size_t)d.nlay, ncol = (size_t)d.ncol, ldu = d.ld > 0 ? (size_t)d.ld : ncol;
    const double *up[NA_IN];
    gcm_pointers(u, two ? (const double *)alpha : nullptr, up);
    std::vector<FormItem> ins, outs;
    for (int a = 0; a < NA_IN; a++) {
        if (a == A_ALPHA ? !two : (CALL_ARRAYS[a].cloud && !cloud)) continue;
        if (!up[a]) return fail(RRTMG_LW_HIP_EARG, a == A_ALPHA ? "icld = 4/5 needs alpha" : "null input array (argument %d of rrtmg_lw's arrays)", a + 1);
        ins.push_back(form_item(up[a], a, L, a == A_TAUCLD ? FA_TAUCLD : FA_PLANE));
    }
    if (!have_outs(uo)) return fail(RRTMG_LW_HIP_EARG, "null output array");
    double *uop[NA_CALL];
    flux_pointers(uo, uop);
    for (int a = A_UFLX; a < A_UFLXS; a++) if (a < A_DUFLX_DT || d.idrv == 1) outs.push_back(form_item(uop[a], a, L));
    const size_t nmean = outs.size();
    // the variance planes: the shape of their means, hr_var flipped with hr
    double *const uvar[3] = {uo.uflx_var, uo.dflx_var, uo.hr_var};
    const int var_of[3] = {A_UFLX, A_DFLX, A_HR};
    int var_item[3] = {-1, -1, -1};
    for (int k = 0; k < 3; k++) if (uvar[k]) { var_item[k] = (int)outs.size(); outs.push_back(form_item(uvar[k], var_of[k], L)); }
    if (*d.icld > 3) *d.icld = 2;                                 // what rrtmg_lw does to the generator's icld (src/rrtmg_lw_rad.f90:469)
    const size_t nbmax = (size_t)balanced_batch(d.ncol, eff_batch(d.nlay));
    if (int rc = ensure_workspace(d.nlay, (int)nbmax, cloud, cloud, d.idrv, mode)) return rc;
    if (cloud) if (int rc = prepare_mask((int)nbmax, d.nlay, icld_gen, 0, (const double *)alpha)) return rc;
    std::vector<double *> si, so;
    const size_t n_in = form_place(ins, nbmax, nullptr, si), n_out = form_place(outs, nbmax, nullptr, so);
    if (int rc = ensure_form(G.form_buf, (n_in + n_out) * 8)) return rc;
    if (int rc = ensure_pipeline()) return rc;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the workspace and the staging
    int rc = 0;
    for (size_t col0 = 0; col0 < ncol && rc == 0; col0 += nbmax) {
        const size_t nb = std::min(nbmax, ncol - col0);
        const size_t used = form_place(ins, nb, G.form_buf.as<double>(), si);
        form_place(outs, nb, G.form_buf.as<double>() + used, so);
        const double *sp[NA_IN] = {};
        for (size_t k = 0; k < ins.size(); k++) sp[ins[k].pos] = si[k];
        double *op[NA_CALL] = {}, *vp[3] = {};
        for (size_t k = 0; k < nmean; k++) op[outs[k].pos] = so[k];
        for (int k = 0; k < 3; k++) if (var_item[k] >= 0) vp[k] = so[(size_t)var_item[k]];
        const FluxOut fo = with_var(flux_from(op), vp[0], vp[1], vp[2]);
        rc = form_launch(s, true, f, ins, si, ldu, col0, nb);
        G.W.mask_col0 = 0;
        if (rc == 0) rc = cloud ? run_samples(s, staged_batch(d, mode, (int)nb), gcm_from(sp), fo, KissGen{true, icld_gen, d.permuteseed, sp[A_ALPHA]}, nsamp, seedstep)
                                : run_batch<true>(s, staged_batch(d, mode, (int)nb), gcm_from(sp), ColIn{}, fo);
        if (rc == 0) rc = form_launch(s, false, f, outs, so, ldu, col0, nb);
    }
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return rc;
}

// (declared in front of run_pipelined) the in-place *_view call with the Mersenne-Twister generator: G.form_gen as above, no conversion
int stage_generator_arrays(hipStream_t s, const CallDesc &d, int icld_gen, const double **play, const double **cldfr, const double **alpha)
{
    const bool two = icld_gen == 4 || icld_gen == 5;
    if (!*play || !*cldfr || (two && !*alpha)) return fail(RRTMG_LW_HIP_EARG, two && !*alpha ? "icld = 4/5 needs alpha" : "null generator input");
    const size_t L = (size_t)d.nlay, n = (size_t)d.ncol;
    std::vector<FormItem> gen = {form_item(*play, A_PLAY, L), form_item(*cldfr, A_CLDFR, L)};
    if (two) gen.push_back(form_item(*alpha, A_ALPHA, L));
    std::vector<double *> sg;
    const size_t need = form_place(gen, n, nullptr, sg);
    if (int rc = ensure_form(G.form_gen, need * 8)) return rc;
    form_place(gen, n, G.form_gen.as<double>(), sg);
    if (int rc = ensure_pipeline()) return rc;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));
    if (int rc = form_launch(s, true, rrtmg_lw_hip_array_form{8, 0, 0}, gen, sg, (size_t)d.ld, 0, n)) return rc;
    *play = sg[0]; *cldfr = sg[1];
    if (two) *alpha = sg[2];
    return 0;
}

int gas_optics_device_as(const rrtmg_lw_hip_array_form &f, int ncol, int nlay, int idrv, const GcmIn &u, const OptOut &uo, void *stream, int ld = 0)
{
    const size_t ldu = ld > 0 ? (size_t)ld : (size_t)ncol;
    ENTRY_LOCK_FOR(u.play);
    if (int rc = check_common(ncol, nlay)) return rc;
    if (int rc = check_optics(idrv, uo)) return rc;
    const size_t L = (size_t)nlay;
    const double *up[NA_IN];
    gcm_pointers(u, nullptr, up);
    std::vector<FormItem> ins, outs;
    for (int a = 0; a <= A_EMIS; a++) {
        if (!up[a]) return fail(RRTMG_LW_HIP_EARG, "gas optics: null input array");
        ins.push_back(form_item(up[a], a, L));
    }
    // (pos: 0 .. 5 = the members of OptOut)
    const auto out = [&](void *p, int pos, int V, int inner, bool vertical) { if (p) outs.push_back(FormItem{p, pos, V, inner, FA_PLANE, vertical}); };
    out(uo.taug, 0, nlay, NGPT, true); out(uo.fracs, 1, nlay, NGPT, true); out(uo.planklay, 2, nlay, NBND, true);
    out(uo.planklev, 3, nlay + 1, NBND, true); out(uo.plankbnd, 4, NBND, 1, false); out(idrv == 1 ? uo.dplankbnd : nullptr, 5, NBND, 1, false);
    // (the outputs are ~40 times a column's inputs: batches of at most ~256 MB of staging each, like the host-pointer entry)
    std::vector<double *> si, so;
    const size_t per_col = (form_place(ins, 1, nullptr, si) + form_place(outs, 1, nullptr, so)) * 8;
    const size_t cap = std::max<size_t>(64, std::min<size_t>((size_t)eff_batch(nlay), ((size_t)256 << 20) / per_col / 64 * 64));
    const size_t nbmax = (size_t)balanced_batch(ncol, (int)std::min<size_t>(cap, (size_t)eff_batch(nlay)));
    if (int rc = ensure_form(G.form_buf, per_col * nbmax)) return rc;
    if (int rc = ensure_pipeline()) return rc;
    if (int rc = ensure_optics_ws(nlay, (int)nbmax)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));
    int rc = 0;
    for (size_t col0 = 0; col0 < (size_t)ncol && rc == 0; col0 += nbmax) {
        const size_t nb = std::min(nbmax, (size_t)ncol - col0);
        const size_t used = form_place(ins, nb, G.form_buf.as<double>(), si);
        form_place(outs, nb, G.form_buf.as<double>() + used, so);
        const double *sp[NA_IN] = {};
        for (size_t k = 0; k < ins.size(); k++) sp[ins[k].pos] = si[k];
        double *op[6] = {};
        for (size_t k = 0; k < outs.size(); k++) op[outs[k].pos] = so[k];
        rc = form_launch(s, true, f, ins, si, ldu, col0, nb);
        Batch b;
        b.nlay = nlay; b.nct = b.nb = (int)nb; b.idrv = idrv;
        if (rc == 0) rc = run_optics<true>(s, b, gcm_from(sp), ColIn{}, OptOut{op[0], op[1], op[2], op[3], op[4], op[5]});
        if (rc == 0) rc = form_launch(s, false, f, outs, so, ldu, col0, nb);
    }
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return rc;
}

// ---- surface-temperature adjustment of idrv = 1 results (rrtmg_lw_hip_adjust_tsfc*, k_adjust_cf / k_adjust_lf) -------------------------
// The arrays of a call as the entries receive them; the clear-sky five all null or all set.
struct AdjustIn { const void *plev, *dtsfc, *uflx, *dflx, *duflx_dt, *uflxc, *dflxc, *duflxc_dt; };
struct AdjustOut { void *uflx_adj, *hr_adj, *uflxc_adj, *hrc_adj; };

// what the three entries check before anything is enqueued; *clear: the clear-sky set is there
int check_adjust(int ncol, int nlay, int real_bytes, const AdjustIn &in, const AdjustOut &o, bool *clear, int ld = 0)
{
    if (int rc = check_common(ncol, nlay)) return rc;
    if (!in.plev || !in.dtsfc || !in.uflx || !in.dflx || !in.duflx_dt) return fail(RRTMG_LW_HIP_EARG, "adjust_tsfc: null input array");
    if (!o.uflx_adj || !o.hr_adj) return fail(RRTMG_LW_HIP_EARG, "adjust_tsfc: null output array");
    const int nc = (in.uflxc != nullptr) + (in.dflxc != nullptr) + (in.duflxc_dt != nullptr) + (o.uflxc_adj != nullptr) + (o.hrc_adj != nullptr);
    if (nc != 0 && nc != 5)
        return fail(RRTMG_LW_HIP_EARG, "adjust_tsfc: uflxc, dflxc, duflxc_dt, uflxc_adj and hrc_adj must be all null or all set (%d of 5 are set)", nc);
    *clear = nc == 5;
    // no output may share a byte with an input or with another output
    // (an array of R rows ld columns apart reaches from the call's first column to its last one in row R - 1)
    const size_t n = (size_t)ncol, w = ld > 0 ? (size_t)ld : n;
    const size_t lev = (w * (size_t)nlay + n) * (size_t)real_bytes, lay = (w * ((size_t)nlay - 1) + n) * (size_t)real_bytes;
    struct Range { const char *name; const void *p; size_t bytes; };
    const Range ins[] = {{"plev", in.plev, lev}, {"dtsfc", in.dtsfc, n * (size_t)real_bytes}, {"uflx", in.uflx, lev}, {"dflx", in.dflx, lev},
                         {"duflx_dt", in.duflx_dt, lev}, {"uflxc", in.uflxc, lev}, {"dflxc", in.dflxc, lev}, {"duflxc_dt", in.duflxc_dt, lev}};
    const Range outs[] = {{"uflx_adj", o.uflx_adj, lev}, {"hr_adj", o.hr_adj, lay}, {"uflxc_adj", o.uflxc_adj, lev}, {"hrc_adj", o.hrc_adj, lay}};
    const auto meet = [](const Range &x, const Range &y) {
        const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
        return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
    };
    for (size_t k = 0; k < 4; k++) {
        for (const Range &i : ins)
            if (meet(outs[k], i)) return fail(RRTMG_LW_HIP_EARG, "adjust_tsfc: output %s overlaps input %s", outs[k].name, i.name);
        for (size_t j = 0; j < k; j++)
            if (meet(outs[k], outs[j])) return fail(RRTMG_LW_HIP_EARG, "adjust_tsfc: output %s overlaps output %s", outs[k].name, outs[j].name);
    }
    return 0;
}

template <class R, bool TOP, int NS>
void adjust_launch_form(hipStream_t s, bool layer_fastest, const AdjustArgs &a, bool aligned)
{
    const size_t n = (size_t)a.ncol;
    if (layer_fastest) {
        constexpr size_t V = 16 / sizeof(R);
        const size_t threads = (n * ((size_t)a.nlay + 1) + V - 1) / V;
        LAUNCH("k_adjust_lf", (k_adjust_lf<R, TOP, NS>), dim3((unsigned)((threads + 255) / 256)), dim3(256), s, a);
        return;
    }
    // 16-byte accesses where every row of every array starts on a 16-byte boundary: the first one does (aligned) and the rows lie a
    // multiple of 16 bytes apart; a call of a *_view entry at an odd column of a field, or with an odd ld, takes the narrow variant
    constexpr size_t V = 16 / sizeof(R);
    const bool wide = aligned && n % V == 0 && (size_t)a.ld % V == 0;
    const size_t threads = wide ? n / V : n;
    // a small call is spread over the chip along the vertical: chunks of at least 8 layers until ~2^18 threads run
    AdjustArgs b = a;
    while (b.chunk > 8 && threads * (size_t)((a.nlay + b.chunk - 1) / b.chunk) < ((size_t)1 << 18)) b.chunk = (b.chunk + 1) / 2;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)((a.nlay + b.chunk - 1) / b.chunk));
    if (wide) LAUNCH("k_adjust_cf", (k_adjust_cf<R, (int)V, TOP, NS>), grid, dim3(256), s, b);
    else LAUNCH("k_adjust_cf", (k_adjust_cf<R, 1, TOP, NS>), grid, dim3(256), s, b);
}

// one launch over ncol columns of arrays that are ncol columns wide - column-fastest ones `ld` columns where ld > 0 -, in the form f, on stream s
int adjust_launch(hipStream_t s, const rrtmg_lw_hip_array_form &f, int ncol, int nlay, const AdjustIn &in, const AdjustOut &o, bool clear, int ld = 0)
{
    AdjustArgs a{};
    a.plev = in.plev; a.dtsfc = in.dtsfc;
    a.s[0] = AdjustSet{in.uflx, in.dflx, in.duflx_dt, o.uflx_adj, o.hr_adj};
    if (clear) a.s[1] = AdjustSet{in.uflxc, in.dflxc, in.duflxc_dt, o.uflxc_adj, o.hrc_adj};
    a.ncol = (unsigned long long)ncol; a.ld = (unsigned long long)(ld > 0 ? ld : ncol); a.nlay = nlay; a.chunk = nlay;
    a.heatfac = G.H.heatfac;
    // column-fastest: rows of ncol values (hr too), the wide path also asks ncol to be a multiple of the vector; layer-fastest: the
    // level arrays as one run from their first byte (dtsfc and hr are accessed value by value)
    const void *all[] = {in.plev, in.dtsfc, in.uflx, in.dflx, in.duflx_dt, o.uflx_adj, o.hr_adj, in.uflxc, in.dflxc, in.duflxc_dt, o.uflxc_adj, o.hrc_adj};
    bool aligned = true;
    for (const void *p : all) aligned = aligned && ((uintptr_t)p & 15u) == 0;
    a.vec = aligned ? 1 : 0;
    const bool lf = f.layer_fastest != 0, top = f.top_first != 0;
#define ADJUST_GO(R)                                                                                     \
    do {                                                                                                 \
        if (top) { if (clear) adjust_launch_form<R, true, 2>(s, lf, a, aligned); else adjust_launch_form<R, true, 1>(s, lf, a, aligned); } \
        else { if (clear) adjust_launch_form<R, false, 2>(s, lf, a, aligned); else adjust_launch_form<R, false, 1>(s, lf, a, aligned); } \
    } while (0)
    if (f.real_bytes == 4) ADJUST_GO(float); else ADJUST_GO(double);
#undef ADJUST_GO
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RRTMG_LW_HIP_EHIP, "k_adjust launch failed: %s", hipGetErrorString(e));
    return 0;
}

int adjust_device(const rrtmg_lw_hip_array_form &f, int ncol, int nlay, const AdjustIn &in, const AdjustOut &o, void *stream, int ld = 0)
{
    ENTRY_LOCK_FOR(in.plev);
    bool clear = false;
    if (int rc = check_adjust(ncol, nlay, f.real_bytes, in, o, &clear, ld)) return rc;
    return adjust_launch((hipStream_t)stream, f, ncol, nlay, in, o, clear, ld);
}

// columns [c0, c1) of a host-pointer call on the calling thread's current device state (the fan-out's worker); no lock taken
int adjust_host_range(int ncol, int c0, int c1, int nlay, const AdjustIn &in, const AdjustOut &o, bool clear, size_t esz = 8)
{
    const size_t L = (size_t)nlay;
    const auto d = [](const void *p) { return static_cast<const double *>(p); };
    std::vector<HostIn> ins = {HostIn{d(in.plev), 1, L + 1, nullptr}, HostIn{d(in.dtsfc), 1, 1, nullptr}, HostIn{d(in.uflx), 1, L + 1, nullptr},
                               HostIn{d(in.dflx), 1, L + 1, nullptr}, HostIn{d(in.duflx_dt), 1, L + 1, nullptr}};
    std::vector<HostOut> outs = {HostOut{static_cast<double *>(o.uflx_adj), L + 1, nullptr, true}, HostOut{static_cast<double *>(o.hr_adj), L, nullptr, true}};
    if (clear) {
        for (const void *p : {in.uflxc, in.dflxc, in.duflxc_dt}) ins.push_back(HostIn{d(p), 1, L + 1, nullptr});
        outs.push_back(HostOut{static_cast<double *>(o.uflxc_adj), L + 1, nullptr, true});
        outs.push_back(HostOut{static_cast<double *>(o.hrc_adj), L, nullptr, true});
    }
    // (esz = 4: the caller's arrays are float; the staged ones, widened, are float64 as ever, and so is the arithmetic)
    for (auto &a : ins) a.esz = esz;
    for (auto &a : outs) a.esz = esz;
    const int nbmax = balanced_batch(c1 - c0, std::min(eff_batch(nlay), HOST_BATCH));
    const rrtmg_lw_hip_array_form ref{8, 0, 0};
    auto body = [&](hipStream_t s, int nb, int, std::vector<HostIn> &i_, std::vector<HostOut> &o_) -> int {
        const AdjustIn si{i_[0].d, i_[1].d, i_[2].d, i_[3].d, i_[4].d, clear ? i_[5].d : nullptr, clear ? i_[6].d : nullptr, clear ? i_[7].d : nullptr};
        const AdjustOut so{o_[0].d, o_[1].d, clear ? o_[2].d : nullptr, clear ? o_[3].d : nullptr};
        return adjust_launch(s, ref, nb, nlay, si, so, clear);
    };
    return host_pipeline(ncol, c0, c1, nbmax, ins, outs, body);
}

}   // namespace

extern "C" {

int rrtmg_lw_hip_adjust_tsfc(int ncol, int nlay, const double *plev, const double *dtsfc,
    const double *uflx, const double *dflx, const double *duflx_dt, const double *uflxc, const double *dflxc, const double *duflxc_dt,
    double *uflx_adj, double *hr_adj, double *uflxc_adj, double *hrc_adj)
{
    ENTRY_LOCK;
    const AdjustIn in{plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt};
    const AdjustOut o{uflx_adj, hr_adj, uflxc_adj, hrc_adj};
    bool clear = false;
    if (int rc = check_adjust(ncol, nlay, 8, in, o, &clear)) return rc;
    return fan_out(ncol, [&](int c0, int c1) { return adjust_host_range(ncol, c0, c1, nlay, in, o, clear); });
}

int rrtmg_lw_hip_adjust_tsfc_r4(int ncol, int nlay, const float *plev, const float *dtsfc,
    const float *uflx, const float *dflx, const float *duflx_dt, const float *uflxc, const float *dflxc, const float *duflxc_dt,
    float *uflx_adj, float *hr_adj, float *uflxc_adj, float *hrc_adj)
{
    ENTRY_LOCK;
    const AdjustIn in{plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt};
    const AdjustOut o{uflx_adj, hr_adj, uflxc_adj, hrc_adj};
    bool clear = false;
    if (int rc = check_adjust(ncol, nlay, 4, in, o, &clear)) return rc;
    return fan_out(ncol, [&](int c0, int c1) { return adjust_host_range(ncol, c0, c1, nlay, in, o, clear, 4); });
}

int rrtmg_lw_hip_adjust_tsfc_device(int ncol, int nlay, const double *plev, const double *dtsfc,
    const double *uflx, const double *dflx, const double *duflx_dt, const double *uflxc, const double *dflxc, const double *duflxc_dt,
    double *uflx_adj, double *hr_adj, double *uflxc_adj, double *hrc_adj, void *stream)
{
    return adjust_device({8, 0, 0}, ncol, nlay, {plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt}, {uflx_adj, hr_adj, uflxc_adj, hrc_adj}, stream);
}

int rrtmg_lw_hip_adjust_tsfc_device_as(const rrtmg_lw_hip_array_form *form, int ncol, int nlay, const void *plev, const void *dtsfc,
    const void *uflx, const void *dflx, const void *duflx_dt, const void *uflxc, const void *dflxc, const void *duflxc_dt,
    void *uflx_adj, void *hr_adj, void *uflxc_adj, void *hrc_adj, void *stream)
{
    bool plain = false;
    if (int rc = form_check(form, &plain)) return rc;
    if (plain) return rrtmg_lw_hip_adjust_tsfc_device(ncol, nlay, (const double *)plev, (const double *)dtsfc, (const double *)uflx, (const double *)dflx,
                                                      (const double *)duflx_dt, (const double *)uflxc, (const double *)dflxc, (const double *)duflxc_dt,
                                                      (double *)uflx_adj, (double *)hr_adj, (double *)uflxc_adj, (double *)hrc_adj, stream);
    return adjust_device(*form, ncol, nlay, {plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt}, {uflx_adj, hr_adj, uflxc_adj, hrc_adj}, stream);
}

#define GCM_PARAMS_AS                                                                                           \
    const void *play, const void *plev, const void *tlay, const void *tlev, const void *tsfc,                   \
    const void *h2ovmr, const void *o3vmr, const void *co2vmr, const void *ch4vmr, const void *n2ovmr,          \
    const void *o2vmr, const void *cfc11vmr, const void *cfc12vmr, const void *cfc22vmr,                        \
    const void *ccl4vmr, const void *emis
#define CLOUD_PARAMS_AS const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp, const void *reice, const void *reliq
#define OUT_PARAMS_AS void *uflx, void *dflx, void *hr, void *uflxc, void *dflxc, void *hrc, void *duflx_dt, void *duflxc_dt

int rrtmg_lw_hip_run_nomcica_device_as(const rrtmg_lw_hip_array_form *form, int ncol, int nlay, int *icld, int idrv, GCM_PARAMS_AS,
    int inflglw, int iceflglw, int liqflglw, CLOUD_PARAMS_AS, const void *tauaer, OUT_PARAMS_AS, void *stream)
{
    bool plain = false;
    if (int rc = form_check(form, &plain)) return rc;
    if (plain) return rrtmg_lw_hip_run_nomcica_device(ncol, nlay, icld, idrv, GCM_NAMES_AS, inflglw, iceflglw, liqflglw, CLOUD_NAMES_AS, AS_(tauaer), OUT_NAMES_AS, stream);
    return nomcica_device_as(*form, {ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw}, {GCM_NAMES_AS, CLOUD_NAMES_AS, AS_(tauaer)}, {OUT_NAMES_AS}, stream);
}

int rrtmg_lw_hip_run_mcica_subcol_device_as(const rrtmg_lw_hip_array_form *form, int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    GCM_PARAMS_AS, int inflglw, int iceflglw, int liqflglw, CLOUD_PARAMS_AS, const void *alpha, const void *tauaer, OUT_PARAMS_AS, void *stream)
{
    bool plain = false;
    if (int rc = form_check(form, &plain)) return rc;
    if (plain) return rrtmg_lw_hip_run_mcica_subcol_device(ncol, nlay, icld, idrv, permuteseed, irng, GCM_NAMES_AS, inflglw, iceflglw, liqflglw,
                                                           CLOUD_NAMES_AS, AS_(alpha), AS_(tauaer), OUT_NAMES_AS, stream);
    return mcica_subcol_device_as(*form, {ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng}, {GCM_NAMES_AS, CLOUD_NAMES_AS, AS_(tauaer)},
                                  alpha, {OUT_NAMES_AS}, stream);
}

int rrtmg_lw_hip_gas_optics_device_as(const rrtmg_lw_hip_array_form *form, int ncol, int nlay, int idrv, GCM_PARAMS_AS,
    void *taug, void *fracs, void *planklay, void *planklev, void *plankbnd, void *dplankbnd_dt, void *stream)
{
    bool plain = false;
    if (int rc = form_check(form, &plain)) return rc;
    if (plain) return rrtmg_lw_hip_gas_optics_device(ncol, nlay, idrv, GCM_NAMES_AS, (double *)taug, (double *)fracs, (double *)planklay,
                                                     (double *)planklev, (double *)plankbnd, (double *)dplankbnd_dt, stream);
    return gas_optics_device_as(*form, ncol, nlay, idrv, {GCM_NAMES_AS},
                                OptOut{(double *)taug, (double *)fracs, (double *)planklay, (double *)planklev, (double *)plankbnd, (double *)dplankbnd_dt}, stream);
}

}  // extern "C"

// ---- device arrays with a column stride (rrtmg_lw_hip_*_view) ---------------------------------------------------------------------------
// The *_as entries' forms plus `ld`: the call's ncol columns lie inside column-fastest arrays ld columns wide, every pointer at the call's
// first column.  Below the entries ld is Batch::nct - the kernels have always taken the batch as (col0, nb) inside arrays nct wide - and
// the call's own column count travels beside it (Batch::ncall; CallDesc::ld above).  The form {8, 0, 0} runs on the caller's arrays in
// place (nomcica_device / mcica_subcol_device / gas_optics_device_ld / adjust_launch with the stride); a converting form goes through
// the *_as staging, whose two kernels take ld as the width of the caller's arrays (FormTable::ncol).
namespace {

constexpr int VIEW_LD_MAX = 1 << 30;          // (include/rrtmg_lw_hip.h: the largest ld)

// what the four entries check first, before any lock is held or anything is launched; *f: the form, *ld: the width in force (ncol for
// 0), *plain: the form {8, 0, 0}
int view_check(const rrtmg_lw_hip_array_view *v, int ncol, rrtmg_lw_hip_array_form *f, int *ld, bool *plain)
{
    if (!v) { ENTRY_LOCK; return fail(RRTMG_LW_HIP_EARG, "array view is null"); }
    *f = rrtmg_lw_hip_array_form{v->real_bytes, v->layer_fastest, v->top_first};
    if (int rc = form_check(f, plain)) return rc;
    *ld = v->ld == 0 ? ncol : v->ld;
    if (ncol < 1) return 0;                     // (refused as a bad dimension by the entry's own checks)
    const char *bad = v->ld < 0 || *ld < ncol ? "array view: ld is smaller than ncol"
                    : *ld > VIEW_LD_MAX ? "array view: ld exceeds 2^30"
                    : (v->layer_fastest && *ld != ncol) ? "array view: with layer_fastest = 1 the column is the slowest index - ld must be 0 or ncol" : nullptr;
    if (bad) { ENTRY_LOCK; return fail(RRTMG_LW_HIP_EARG, "%s (ld=%d, ncol=%d)", bad, v->ld, ncol); }
    return 0;
}

// ---- cloud cover as the sub-columns realise it (rrtmg_lw_hip_mcica_cloud_cover*, k_cloudcover) -----------------------------------------
// The generator stage of the fused entries - prepare_mask / launch_kiss with the seeds permuteseed + i seedstep, or generate_mask for
// the Mersenne Twister - for ALL columns of the call at once, and per sample one k_cloudcover launch that counts the mask into the
// caller's arrays.  No solver kernel runs; the mask buffer is the fused entries' (G.mask), so the call ends in G.ev_last like theirs.
struct CoverOut { void *cldtot, *cldcum, *cldlay; unsigned *submask; };

// what the three entries check, in this order, before anything is allocated or enqueued (the pointers: the caller's, host or device)
int check_cover(int ncol, int nlay, int icld, int permuteseed, int nsamp, int seedstep, int *irng, const void *play, const void *cldfr,
                const void *alpha, const CoverOut &o)
{
    if (int rc = check_mcica_build()) return rc;
    if (int rc = check_subcol_args(ncol, nlay, icld, irng)) return rc;
    CallDesc d{ncol, nlay, nullptr, 0, 0, 0, 0, permuteseed, irng};
    if (int rc = check_samples(d, nsamp, seedstep)) return rc;
    if (!o.cldtot && !o.cldcum && !o.cldlay && !o.submask)
        return fail(RRTMG_LW_HIP_EARG, "cloud cover: cldtot, cldcum, cldlay and submask are all null - at least one output");
    if (o.submask && nsamp > 1) return fail(RRTMG_LW_HIP_EARG, "cloud cover: submask with nsamp = %d: the mask is that of ONE sample (pass NULL, or nsamp = 1)", nsamp);
    if (icld == 0) return 0;                                      // (nothing is drawn, nothing is read)
    if (!play) return fail(RRTMG_LW_HIP_EARG, "cloud cover: null input array (play)");
    if (!cldfr) return fail(RRTMG_LW_HIP_EARG, "cloud cover: null input array (cldfr)");
    if ((icld == 4 || icld == 5) && !alpha) return fail(RRTMG_LW_HIP_EARG, "icld = 4/5 needs alpha");
    if (nlay < 4 && *irng == 0) return fail(RRTMG_LW_HIP_EARG, "the kissvec generator needs at least four layers");
    return 0;
}

// the call on stream s from DEVICE arrays in the form f, ld columns wide; checked (check_cover), the caller holds the entry lock
int cover_launch(const rrtmg_lw_hip_array_form &f, int ncol, int nlay, int ld, int icld, int permuteseed, int nsamp, int seedstep, int irng,
                 const void *play, const void *cldfr, const void *alpha, const CoverOut &o, hipStream_t s)
{
    const bool cloud = icld != 0, two = icld == 4 || icld == 5;
    const bool plain = f.real_bytes == 8 && !f.layer_fastest && !f.top_first;
    const size_t L = (size_t)nlay, n = (size_t)ncol;
    if (int rc = ensure_pipeline()) return rc;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the mask and the staging
    // the generator's inputs: the caller's own where they are float64 reference-form arrays - the kissvec kernels take their width, the
    // Mersenne-Twister ones arrays as wide as the call -, staged call-wide otherwise, as the fused *_view entries stage them
    const double *gp = (const double *)play, *gc = (const double *)cldfr, *ga = two ? (const double *)alpha : nullptr;
    int gw = ld;
    if (cloud && (!plain || (irng != 0 && ld != ncol))) {
        std::vector<FormItem> gen = {form_item(play, A_PLAY, L), form_item(cldfr, A_CLDFR, L)};
        if (two) gen.push_back(form_item(alpha, A_ALPHA, L));
        std::vector<double *> sg;
        const size_t need = form_place(gen, n, nullptr, sg);
        if (int rc = ensure_form(G.form_gen, need * 8)) return rc;
        form_place(gen, n, G.form_gen.as<double>(), sg);
        if (int rc = form_launch(s, true, f, gen, sg, (size_t)ld, 0, n)) return rc;
        gp = sg[0]; gc = sg[1]; ga = two ? sg[2] : nullptr;
        gw = ncol;
    }
    if (cloud && irng == 0) if (int rc = prepare_mask(ncol, nlay, icld, 0, ga)) return rc;
    CoverArgs a{};
    a.cldtot = o.cldtot; a.cldcum = o.cldcum; a.cldlay = o.cldlay; a.submask = o.submask;
    a.ncol = (unsigned long long)ncol; a.ld = (unsigned long long)ld;
    a.nlay = nlay; a.layer_fastest = f.layer_fastest; a.top_first = f.top_first;
    a.cloud = cloud ? 1 : 0;
    const int ns = cloud ? nsamp : 1;                             // (no cloud: every sample is the same zeros)
    a.denom = (double)(NGPT * ns);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    for (int i = 0; i < ns; i++) {
        const int seed = (int)((long long)permuteseed + (long long)i * seedstep);
        if (cloud && irng == 0) { if (int rc = launch_kiss(s, G.W, gw, 0, ncol, nlay, icld, seed, SubcolIn{gp, gc, ga})) return rc; }
        else if (cloud) { if (int rc = generate_mask(s, ncol, nlay, icld, seed, irng, gp, gc, ga)) return rc; }
        a.first = i == 0; a.last = i == ns - 1;
        if (f.real_bytes == 4) LAUNCH("k_cloudcover<f32>", (k_cloudcover<float>), grid, block, s, G.W, a);
        else LAUNCH("k_cloudcover<f64>", (k_cloudcover<double>), grid, block, s, G.W, a);
    }
    if (int rc = launches_ok()) return rc;
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return 0;
}

int cover_device(const rrtmg_lw_hip_array_form &f, int ncol, int nlay, int ld, int icld, int permuteseed, int nsamp, int seedstep, int *irng,
                 const void *play, const void *cldfr, const void *alpha, const CoverOut &o, void *stream)
{
    // (icld = 0 reads no array: the outputs say where the call runs)
    const void *where = play ? play : o.cldtot ? o.cldtot : o.cldcum ? o.cldcum : o.cldlay ? o.cldlay : (const void *)o.submask;
    ENTRY_LOCK_FOR(where, irng && *irng != 0);
    if (int rc = check_cover(ncol, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, o)) return rc;
    return cover_launch(f, ncol, nlay, ld, icld, permuteseed, nsamp, seedstep, *irng, play, cldfr, alpha, o, (hipStream_t)stream);
}

// ---- cloud optics (rrtmg_lw_hip_cloud_optics*, k_cloudoptics_col / k_cloudoptics) ---------------------------------------------------------
// cldprop's / cldprmc's optical depth per spectral band before the diffusivity secant, cldprop's band count and the secants, formed by two
// kernels of their own straight from and into the caller's arrays in the caller's form; no solver kernel runs and none is shared.  The
// one piece of workspace is the band-count walk's (nlay + 1) bytes per column, at the head of the *_as staging buffer (G.form_buf).
struct CloudOpticsIn { const void *cldfr, *taucld, *cicewp, *cliqwp, *reice, *reliq, *plev, *h2ovmr; };
struct CloudOpticsOut { void *taucloud; int *ncbands; void *secdiff; };

// what the three entries check, in this order, before anything is allocated or enqueued (the pointers: the caller's, host or device);
// ld: the column extent of the arrays, real_bytes: their element size
int check_cloud_optics(int ncol, int nlay, int ld, int real_bytes, int imca, const CloudOpticsIn &in, const CloudOpticsOut &o)
{
    if (int rc = check_common(ncol, nlay)) return rc;
    if (imca != 0 && imca != 1) return fail(RRTMG_LW_HIP_EARG, "cloud optics: imca = %d - 0 (cldprop) or 1 (cldprmc)", imca);
    if (!o.taucloud && !o.ncbands && !o.secdiff)
        return fail(RRTMG_LW_HIP_EARG, "cloud optics: taucloud, ncbands and secdiff are all null - at least one output");
    struct Range { const char *name; const void *p; size_t bytes; bool need; };
    const size_t n = (size_t)ncol, w = (size_t)ld, L = (size_t)nlay, rb = (size_t)real_bytes;
    const bool cloud = o.taucloud || o.ncbands, sec = o.secdiff != nullptr;
    // (an array of R rows ld columns apart reaches from the call's first column to its last one in row R - 1)
    const size_t lay = (w * (L - 1) + n) * rb, lev = (w * L + n) * rb;
    const Range ins[] = {{"cldfr", in.cldfr, lay, cloud}, {"taucld", in.taucld, NBND * lay, cloud}, {"cicewp", in.cicewp, lay, cloud},
                         {"cliqwp", in.cliqwp, lay, cloud}, {"reice", in.reice, lay, cloud}, {"reliq", in.reliq, lay, cloud},
                         {"plev", in.plev, lev, sec}, {"h2ovmr", in.h2ovmr, lay, sec}};
    const Range outs[] = {{"taucloud", o.taucloud, (w * (L * NBND - 1) + n) * rb, false}, {"ncbands", o.ncbands, n * sizeof(int), false},
                          {"secdiff", o.secdiff, (w * (NBND - 1) + n) * rb, false}};
    for (const Range &i : ins)
        if (i.need && !i.p) return fail(RRTMG_LW_HIP_EARG, "cloud optics: null input array (%s)", i.name);
    const auto meet = [](const Range &x, const Range &y) {
        const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
        return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
    };
    for (size_t k = 0; k < 3; k++) {
        for (const Range &i : ins)
            if (i.need && meet(outs[k], i)) return fail(RRTMG_LW_HIP_EARG, "cloud optics: output %s overlaps input %s", outs[k].name, i.name);
        for (size_t j = 0; j < k; j++)
            if (meet(outs[k], outs[j])) return fail(RRTMG_LW_HIP_EARG, "cloud optics: output %s overlaps output %s", outs[k].name, outs[j].name);
    }
    return 0;
}

// the call on stream s from DEVICE arrays in the form f, ld columns wide; checked (check_cloud_optics), the caller holds the entry lock
int cloud_optics_launch(const rrtmg_lw_hip_array_form &f, int ncol, int nlay, int ld, int imca, int inflag, int iceflag, int liqflag,
                        const CloudOpticsIn &in, const CloudOpticsOut &o, hipStream_t s)
{
    const bool cloud = o.taucloud || o.ncbands;
    if (int rc = ensure_pipeline()) return rc;
    if (cloud) if (int rc = ensure_form(G.form_buf, ((size_t)nlay + 1) * (size_t)ncol)) return rc;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the staging buffer
    CloudOpticsArgs a{};
    if (cloud) { a.cldfr = in.cldfr; a.taucld = in.taucld; a.cicewp = in.cicewp; a.cliqwp = in.cliqwp; a.reice = in.reice; a.reliq = in.reliq; }
    if (o.secdiff) { a.plev = in.plev; a.h2ovmr = in.h2ovmr; }
    a.taucloud = o.taucloud; a.secdiff = o.secdiff; a.ncbands = o.ncbands;
    a.nbat = cloud ? G.form_buf.as<unsigned char>() : nullptr;
    a.ncol = (unsigned long long)ncol; a.ld = (unsigned long long)ld;
    a.nlay = nlay; a.layer_fastest = f.layer_fastest; a.top_first = f.top_first;
    a.imca = imca; a.inflag = inflag; a.iceflag = iceflag; a.liqflag = liqflag;
    a.err = G.d_err.as<int>();
    // (thread-per-column: one wave per workgroup, so that a call of one wave per 64 columns spreads over the CUs - run_prep)
    const dim3 cgrid((unsigned)(((size_t)ncol + 63) / 64)), cblock(64);
    const dim3 lgrid((unsigned)(((size_t)ncol + BLOCK - 1) / BLOCK), (unsigned)nlay), lblock(BLOCK);
    if (f.real_bytes == 4) {
        LAUNCH("k_cloudoptics_col<f32>", (k_cloudoptics_col<float>), cgrid, cblock, s, a);
        if (cloud) LAUNCH("k_cloudoptics<f32>", (k_cloudoptics<float>), lgrid, lblock, s, G.D, a);
    } else {
        LAUNCH("k_cloudoptics_col<f64>", (k_cloudoptics_col<double>), cgrid, cblock, s, a);
        if (cloud) LAUNCH("k_cloudoptics<f64>", (k_cloudoptics<double>), lgrid, lblock, s, G.D, a);
    }
    if (int rc = launches_ok()) return rc;
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return 0;
}

int cloud_optics_device(const rrtmg_lw_hip_array_form &f, int ncol, int nlay, int ld, int imca, int inflag, int iceflag, int liqflag,
                        const CloudOpticsIn &in, const CloudOpticsOut &o, void *stream)
{
    ENTRY_LOCK_FOR(in.cldfr ? in.cldfr : in.plev);
    if (int rc = check_cloud_optics(ncol, nlay, ld, f.real_bytes, imca, in, o)) return rc;
    return cloud_optics_launch(f, ncol, nlay, ld, imca, inflag, iceflag, liqflag, in, o, (hipStream_t)stream);
}

// ---- the solver on the caller's optical depths and sources (rrtmg_lw_hip_solve*, k_solve / k_solve_flux) -----------------------------------
// rtrn's / rtrnmc's level loops in float64 by two kernels of their own; the one piece of workspace is the per-band partial sums of a
// column batch, at the head of the *_as staging buffer (G.form_buf).
struct SolveIn { const double *plev, *emis, *tau, *fracs, *planklay, *planklev, *plankbnd, *dplankbnd_dt, *cldfr, *odcld; const unsigned *submask; };
struct SolveOut { double *uflx, *dflx, *hr, *uflxc, *dflxc, *hrc, *duflx_dt, *duflxc_dt; };

// what both entries check, in this order, before anything is allocated or enqueued (the pointers: the caller's, host or device)
int check_solve(int ncol, int nlay, int cloud, int idrv, const SolveIn &in, const SolveOut &o)
{
    if (int rc = check_common(ncol, nlay)) return rc;
    if (cloud < 0 || cloud > 2) return fail(RRTMG_LW_HIP_EARG, "solve: cloud = %d - 0 (none), 1 (rtrn: cldfr, odcld) or 2 (rtrnmc: submask, odcld)", cloud);
    if (idrv != 0 && idrv != 1) return fail(RRTMG_LW_HIP_EARG, "solve: idrv = %d - 0 or 1", idrv);
    struct Range { const char *name; const void *p; size_t bytes; bool need; };
    const size_t n = (size_t)ncol, L = (size_t)nlay;
    const size_t lay = n * L * 8, lev = n * (L + 1) * 8, bnd = n * NBND * 8;
    const Range ins[] = {{"plev", in.plev, lev, true}, {"emis", in.emis, bnd, true}, {"tau", in.tau, lay * NGPT, true}, {"fracs", in.fracs, lay * NGPT, true},
                         {"planklay", in.planklay, lay * NBND, true}, {"planklev", in.planklev, lev * NBND, true}, {"plankbnd", in.plankbnd, bnd, true},
                         {"dplankbnd_dt", in.dplankbnd_dt, bnd, idrv == 1}, {"cldfr", in.cldfr, lay, cloud == 1}, {"odcld", in.odcld, lay * NBND, cloud != 0},
                         {"submask", in.submask, n * L * MASK_WORDS * sizeof(unsigned), cloud == 2}};
    const Range outs[] = {{"uflx", o.uflx, lev, true}, {"dflx", o.dflx, lev, true}, {"hr", o.hr, lay, true}, {"uflxc", o.uflxc, lev, false},
                          {"dflxc", o.dflxc, lev, false}, {"hrc", o.hrc, lay, false}, {"duflx_dt", o.duflx_dt, lev, idrv == 1}, {"duflxc_dt", o.duflxc_dt, lev, idrv == 1}};
    for (const Range &i : ins)
        if (i.need && !i.p) return fail(RRTMG_LW_HIP_EARG, "solve: null input array (%s)", i.name);
    for (const Range &x : outs)
        if (x.need && !x.p) return fail(RRTMG_LW_HIP_EARG, "solve: null output array (%s)", x.name);
    if ((!o.uflxc || !o.dflxc || !o.hrc) && (o.uflxc || o.dflxc || o.hrc))
        return fail(RRTMG_LW_HIP_EARG, "solve: uflxc, dflxc and hrc must be all null or all set (%s is null)", !o.uflxc ? "uflxc" : !o.dflxc ? "dflxc" : "hrc");
    const auto meet = [](const Range &x, const Range &y) {
        const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
        return x.p && y.p && a < b + y.bytes && b < a + x.bytes;
    };
    for (size_t k = 0; k < 8; k++) {
        if (k >= 6 && idrv != 1) continue;                  // (not formed, not touched)
        for (const Range &i : ins)
            if (i.need && meet(outs[k], i)) return fail(RRTMG_LW_HIP_EARG, "solve: output %s overlaps input %s", outs[k].name, i.name);
        for (size_t j = 0; j < k; j++)
            if (meet(outs[k], outs[j])) return fail(RRTMG_LW_HIP_EARG, "solve: output %s overlaps output %s", outs[k].name, outs[j].name);
    }
    return 0;
}

// the slots of the per-band partials a call forms: without cloud the clear-sky stream is the total one
int solve_slots(int cloud, int idrv, int *slot)
{
    const bool own = cloud != 0;
    slot[SV_U] = 0; slot[SV_D] = 1;
    slot[SV_UC] = own ? 2 : 0; slot[SV_DC] = own ? 3 : 1;
    const int n = own ? 4 : 2;
    slot[SV_DU] = idrv == 1 ? n : -1;
    slot[SV_DUC] = idrv == 1 ? (own ? n + 1 : n) : -1;
    return n + (idrv == 1 ? (own ? 2 : 1) : 0);
}

// ncol columns on stream s from DEVICE arrays ld columns wide, in batches of at most nbmax columns; checked (check_solve), the caller holds
// the entry lock
int solve_launch(int ncol, int nlay, int ld, int nbmax, int cloud, int idrv, const SolveIn &in, const SolveOut &o, hipStream_t s)
{
    if (int rc = ensure_pipeline()) return rc;
    SolveArgs a{};
    const int nslot = solve_slots(cloud, idrv, a.slot);
    const size_t L = (size_t)nlay, nbm = (size_t)std::min(ncol, nbmax);
    if (int rc = ensure_form(G.form_buf, (size_t)nslot * NBND * (L + 1) * nbm * 8)) return rc;
    if (G.ev_last_valid) HIP_TRY(hipStreamWaitEvent(s, G.ev_last.get(), 0));      // an earlier call, possibly on another stream, still owns the staging buffer
    a.part = G.form_buf.as<double>();
    a.ld = (unsigned long long)ld; a.nlay = nlay; a.cloud = cloud;
    for (size_t c0 = 0; c0 < (size_t)ncol; c0 += nbm) {
        const size_t nb = std::min(nbm, (size_t)ncol - c0);
        const auto at = [&](const double *p) { return p ? p + c0 : nullptr; };
        a.plev = at(in.plev); a.emis = at(in.emis); a.tau = at(in.tau); a.fracs = at(in.fracs); a.planklay = at(in.planklay); a.planklev = at(in.planklev);
        a.plankbnd = at(in.plankbnd); a.dplankbnd_dt = idrv == 1 ? at(in.dplankbnd_dt) : nullptr;
        a.cldfr = cloud == 1 ? at(in.cldfr) : nullptr; a.odcld = cloud != 0 ? at(in.odcld) : nullptr;
        a.submask = cloud == 2 ? in.submask + c0 : nullptr;
        const auto ot = [&](double *p) { return p ? p + c0 : nullptr; };
        a.uflx = ot(o.uflx); a.dflx = ot(o.dflx); a.hr = ot(o.hr); a.uflxc = ot(o.uflxc); a.dflxc = ot(o.dflxc); a.hrc = ot(o.hrc);
        a.duflx_dt = idrv == 1 ? ot(o.duflx_dt) : nullptr; a.duflxc_dt = idrv == 1 ? ot(o.duflxc_dt) : nullptr;
        a.nb = (unsigned long long)nb;
        // (one wave per workgroup: a call of one wave per 64 columns and band spreads over the CUs)
        const dim3 grid((unsigned)((nb + 63) / 64), NBND), cgrid((unsigned)((nb + 63) / 64)), block(64);
        if (idrv == 1) LAUNCH("k_solve<1>", (k_solve<1>), grid, block, s, G.D, a);
        else LAUNCH("k_solve<0>", (k_solve<0>), grid, block, s, G.D, a);
        LAUNCH("k_solve_flux", k_solve_flux, cgrid, block, s, G.D, a);
    }
    if (int rc = launches_ok()) return rc;
    HIP_TRY(hipEventRecord(G.ev_last.get(), s));
    G.ev_last_valid = true;
    return 0;
}

}   // namespace

extern "C" {

#define SPEC_PARAMS_AS void *uflxs, void *dflxs, void *uflxcs, void *dflxcs
#define SPEC_NAMES_AS nullptr, nullptr, (double *)uflxs, (double *)dflxs, (double *)uflxcs, (double *)dflxcs

int rrtmg_lw_hip_run_nomcica_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int *icld, int idrv, GCM_PARAMS_AS,
    int inflglw, int iceflglw, int liqflglw, CLOUD_PARAMS_AS, const void *tauaer, OUT_PARAMS_AS, SPEC_PARAMS_AS, void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    CallDesc d{ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw};
    d.spectral = uflxs || dflxs || uflxcs || dflxcs;
    d.ld = ld;
    const GcmIn g{GCM_NAMES_AS, CLOUD_NAMES_AS, AS_(tauaer)};
    const FluxOut out{OUT_NAMES_AS, SPEC_NAMES_AS};
    if (plain) return nomcica_device(d, g, out, stream);          // (ld = ncol: what the plain / spectral device entry does)
    return nomcica_device_as(f, d, g, out, stream);
}

int rrtmg_lw_hip_run_mcica_subcol_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int *icld, int idrv, int permuteseed, int *irng,
    GCM_PARAMS_AS, int inflglw, int iceflglw, int liqflglw, CLOUD_PARAMS_AS, const void *alpha, const void *tauaer, OUT_PARAMS_AS, SPEC_PARAMS_AS,
    void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    CallDesc d{ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng};
    d.spectral = uflxs || dflxs || uflxcs || dflxcs;
    d.ld = ld;
    const GcmIn g{GCM_NAMES_AS, CLOUD_NAMES_AS, AS_(tauaer)};
    const FluxOut out{OUT_NAMES_AS, SPEC_NAMES_AS};
    if (plain) return mcica_subcol_device(d, g, AS_(alpha), out, stream);
    return mcica_subcol_device_as(f, d, g, alpha, out, stream);
}

// The mean over nsamp samples, and optionally the sample variances, of DEVICE arrays in the caller's own form and width.  {8, 0, 0, ld}
// runs in place (run_samples: Batch::nct is the stride); a converting form stages per batch (mcica_samples_as_run); a single sample is
// rrtmg_lw_hip_run_mcica_subcol_device_view.
int rrtmg_lw_hip_run_mcica_samples_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int *icld, int idrv, int permuteseed, int nsamp,
    int seedstep, int *irng, GCM_PARAMS_AS, int inflglw, int iceflglw, int liqflglw, CLOUD_PARAMS_AS, const void *alpha, const void *tauaer, OUT_PARAMS_AS,
    void *uflx_var, void *dflx_var, void *hr_var, void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    CallDesc d{ncol, nlay, icld, idrv, inflglw, iceflglw, liqflglw, permuteseed, irng};
    d.ld = ld;
    const GcmIn g{GCM_NAMES_AS, CLOUD_NAMES_AS, AS_(tauaer)};
    const FluxOut out = with_var({OUT_NAMES_AS}, (double *)uflx_var, (double *)dflx_var, (double *)hr_var);
    {
        ENTRY_LOCK_FOR(play, irng && *irng != 0);
        if (int rc = check_samples(d, nsamp, seedstep)) return rc;
        // (what an array spans: its last row ends ncol, not ld, columns in; layer-fastest arrays have ld = ncol)
        const auto span = [&](size_t rows) { return rows == 0 || ncol < 1 ? (size_t)0 : ((rows - 1) * (size_t)ld + (size_t)ncol) * (size_t)f.real_bytes; };
        if (int rc = check_var(out, nsamp, span((size_t)std::max(nlay, 0) + 1), span((size_t)std::max(nlay, 0)))) return rc;
        if (plain) return mcica_subcol_device_run(d, g, AS_(alpha), out, (hipStream_t)stream, nsamp, seedstep);
        if (nsamp > 1) return mcica_samples_as_run(f, d, g, alpha, out, nsamp, seedstep, (hipStream_t)stream);
    }
    return mcica_subcol_device_as(f, d, g, alpha, out, stream);      // (one sample, no variance: the entry takes the lock itself)
}

// alpha of the exponential overlaps from DEVICE arrays in the caller's form, on the caller's stream, no synchronisation (k_alpha_view)
int rrtmg_lw_hip_get_alpha_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int icld, int idcor, double decorr_con,
    const void *dz, const void *lat, int juldat, const void *cldfrac, void *alpha, void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    ENTRY_LOCK_FOR(dz);
    if (int rc = check_common(ncol, nlay)) return rc;
    if (!(icld == 4 || icld == 5)) return 0;                      // alpha is only defined for the exponential overlaps
    if (!dz || !cldfrac || (idcor == 1 && !lat)) return fail(RRTMG_LW_HIP_EARG, "null input array (%s)", !dz ? "dz" : !cldfrac ? "cldfrac" : "lat");
    if (!alpha) return fail(RRTMG_LW_HIP_EARG, "null output array (alpha)");
    const dim3 grid((ncol + BLOCK - 1) / BLOCK, nlay), block(BLOCK);
    hipStream_t s = (hipStream_t)stream;
    if (f.real_bytes == 4)
        LAUNCH("k_alpha_view<f32>", (k_alpha_view<float>), grid, block, s, ncol, nlay, (size_t)ld, f.layer_fastest, f.top_first, icld, idcor, decorr_con,
               (const float *)dz, (const float *)lat, juldat, (const float *)cldfrac, (float *)alpha);
    else
        LAUNCH("k_alpha_view<f64>", (k_alpha_view<double>), grid, block, s, ncol, nlay, (size_t)ld, f.layer_fastest, f.top_first, icld, idcor, decorr_con,
               (const double *)dz, (const double *)lat, juldat, (const double *)cldfrac, (double *)alpha);
    return launches_ok();
}

// Cloud cover as the McICA sub-columns realise it: DEVICE arrays in the reference form ...
int rrtmg_lw_hip_mcica_cloud_cover_device(int ncol, int nlay, int icld, int permuteseed, int nsamp, int seedstep, int *irng,
    const double *play, const double *cldfr, const double *alpha, double *cldtot, double *cldcum, double *cldlay, unsigned *submask, void *stream)
{
    return cover_device({8, 0, 0}, ncol, nlay, ncol, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, {cldtot, cldcum, cldlay, submask}, stream);
}
// ... in the caller's form and width ({8, 0, 0, ld}: in place) ...
int rrtmg_lw_hip_mcica_cloud_cover_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int icld, int permuteseed, int nsamp,
    int seedstep, int *irng, const void *play, const void *cldfr, const void *alpha, void *cldtot, void *cldcum, void *cldlay, unsigned *submask,
    void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    return cover_device(f, ncol, nlay, ld, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, {cldtot, cldcum, cldlay, submask}, stream);
}
// ... and HOST arrays: the first device, the call's arrays in one per-call device allocation, the outputs copied back
int rrtmg_lw_hip_mcica_cloud_cover(int ncol, int nlay, int icld, int permuteseed, int nsamp, int seedstep, int *irng,
    const double *play, const double *cldfr, const double *alpha, double *cldtot, double *cldcum, double *cldlay, unsigned *submask)
{
    ENTRY_LOCK;
    const CoverOut ho{cldtot, cldcum, cldlay, submask};
    if (int rc = check_cover(ncol, nlay, icld, permuteseed, nsamp, seedstep, irng, play, cldfr, alpha, ho)) return rc;
    HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the workspace
    const size_t n = (size_t)ncol, cells = n * (size_t)nlay;
    const bool cloud = icld != 0, two = icld == 4 || icld == 5;
    const double *hin[3] = {cloud ? play : nullptr, cloud ? cldfr : nullptr, two ? alpha : nullptr};
    double *hout[3] = {cldtot, cldcum, cldlay};
    const size_t nout[3] = {n, cells, cells};
    size_t bytes = 0;
    for (int k = 0; k < 3; k++) bytes += (hin[k] ? cells : 0) * 8 + (hout[k] ? nout[k] : 0) * 8;
    if (submask) bytes += cells * MASK_WORDS * sizeof(unsigned);
    DevBuf buf;                             // (released when the call is left, on every path)
    if (int rc = grow(buf, bytes, bytes, "arrays of a cloud-cover call")) return rc;
    const double *din[3] = {};
    double *dout[3] = {};
    double *p = buf.as<double>();
    for (int k = 0; k < 3; k++) if (hin[k]) { if (int rc = bounce_h2d(p, hin[k], cells * 8)) return rc; din[k] = p; p += cells; }
    for (int k = 0; k < 3; k++) if (hout[k]) { dout[k] = p; p += nout[k]; }
    unsigned *const dmask = submask ? reinterpret_cast<unsigned *>(p) : nullptr;
    hipStream_t s = G.stream.get();
    if (int rc = cover_launch({8, 0, 0}, ncol, nlay, ncol, icld, permuteseed, nsamp, seedstep, *irng, din[0], din[1], din[2], {dout[0], dout[1], dout[2], dmask}, s)) return rc;
    if (int rc = read_physics_error(s)) return rc;
    for (int k = 0; k < 3; k++) if (hout[k]) { if (int rc = bounce_d2h(hout[k], dout[k], nout[k] * 8)) return rc; }
    if (submask) { if (int rc = bounce_d2h(submask, dmask, cells * MASK_WORDS * sizeof(unsigned))) return rc; }
    return 0;
}

// Cloud optics - cldprop's / cldprmc's optical depths per spectral band, the band count, the diffusivity secants: DEVICE arrays in the
// reference form ...
int rrtmg_lw_hip_cloud_optics_device(int ncol, int nlay, int imca, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp, const double *reice, const double *reliq,
    const double *plev, const double *h2ovmr, double *taucloud, int *ncbands, double *secdiff, void *stream)
{
    return cloud_optics_device({8, 0, 0}, ncol, nlay, ncol, imca, inflglw, iceflglw, liqflglw,
                               {cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr}, {taucloud, ncbands, secdiff}, stream);
}
// ... in the caller's form and width (every form runs on the caller's arrays: nothing is staged) ...
int rrtmg_lw_hip_cloud_optics_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int imca, int inflglw, int iceflglw, int liqflglw,
    const void *cldfr, const void *taucld, const void *cicewp, const void *cliqwp, const void *reice, const void *reliq,
    const void *plev, const void *h2ovmr, void *taucloud, int *ncbands, void *secdiff, void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    return cloud_optics_device(f, ncol, nlay, ld, imca, inflglw, iceflglw, liqflglw,
                               {cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr}, {taucloud, ncbands, secdiff}, stream);
}
// ... and HOST arrays: the first device, column batches through the host-entry staging buffer (a column's values do not depend on its
// neighbours, so the results do not depend on the batch size)
int rrtmg_lw_hip_cloud_optics(int ncol, int nlay, int imca, int inflglw, int iceflglw, int liqflglw,
    const double *cldfr, const double *taucld, const double *cicewp, const double *cliqwp, const double *reice, const double *reliq,
    const double *plev, const double *h2ovmr, double *taucloud, int *ncbands, double *secdiff)
{
    ENTRY_LOCK;
    if (int rc = check_cloud_optics(ncol, nlay, ncol, 8, imca, {cldfr, taucld, cicewp, cliqwp, reice, reliq, plev, h2ovmr}, {taucloud, ncbands, secdiff})) return rc;
    HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the staging
    const size_t n = (size_t)ncol, L = (size_t)nlay;
    const bool cloud = taucloud || ncbands, sec = secdiff != nullptr;
    const auto in = [](const double *p, bool on, size_t inner, size_t rows) { return HostIn{on ? p : nullptr, inner, rows, nullptr}; };
    std::vector<HostIn> ins = {in(cldfr, cloud, 1, L), in(taucld, cloud, NBND, L), in(cicewp, cloud, 1, L), in(cliqwp, cloud, 1, L),
                               in(reice, cloud, 1, L), in(reliq, cloud, 1, L), in(plev, sec, 1, L + 1), in(h2ovmr, sec, 1, L)};
    // (ncbands: int32, one 8-byte slot per column in the staging; copied back by hand below - h stays null for stage_out)
    std::vector<HostOut> outs = {HostOut{taucloud, taucloud ? NBND * L : 0, nullptr, taucloud != nullptr}, HostOut{nullptr, ncbands ? (size_t)1 : 0, nullptr, false},
                                 HostOut{secdiff, sec ? (size_t)NBND : 0, nullptr, sec}};
    const int nbmax = balanced_batch(ncol, std::min(eff_batch(nlay), HOST_BATCH));
    if (int rc = stage_alloc(ins, outs, (size_t)nbmax)) return rc;
    hipStream_t s = G.stream.get();
    for (size_t col0 = 0; col0 < n; col0 += (size_t)nbmax) {
        const size_t nb = std::min((size_t)nbmax, n - col0);
        if (int rc = stage_in(ins, n, col0, nb, s)) return rc;
        int *const dnb = ncbands ? reinterpret_cast<int *>(outs[1].d) : nullptr;
        if (int rc = cloud_optics_launch({8, 0, 0}, (int)nb, nlay, (int)nb, imca, inflglw, iceflglw, liqflglw,
                                         {ins[0].d, ins[1].d, ins[2].d, ins[3].d, ins[4].d, ins[5].d, ins[6].d, ins[7].d},
                                         {taucloud ? outs[0].d : nullptr, dnb, sec ? outs[2].d : nullptr}, s)) return rc;
        if (int rc = read_physics_error(s)) return rc;
        if (int rc = stage_out(outs, n, col0, nb, s)) return rc;
        if (ncbands) { if (int rc = bounce_d2h(ncbands + col0, dnb, nb * sizeof(int))) return rc; }
    }
    return 0;
}

// The solver on the caller's optical depths and sources - rtrn's / rtrnmc's level loops, fluxes and heating rates: DEVICE arrays in the
// reference form, column batches of rrtmg_lw_hip_effective_batch(nlay) ...
int rrtmg_lw_hip_solve_device(int ncol, int nlay, int cloud, int idrv, const double *plev, const double *emis, const double *tau, const double *fracs,
    const double *planklay, const double *planklev, const double *plankbnd, const double *dplankbnd_dt, const double *cldfr, const double *odcld,
    const unsigned *submask, double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc, double *duflx_dt, double *duflxc_dt,
    void *stream)
{
    ENTRY_LOCK_FOR(tau);
    const SolveIn in{plev, emis, tau, fracs, planklay, planklev, plankbnd, dplankbnd_dt, cldfr, odcld, submask};
    const SolveOut o{uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt};
    if (int rc = check_solve(ncol, nlay, cloud, idrv, in, o)) return rc;
    return solve_launch(ncol, nlay, ncol, eff_batch(nlay), cloud, idrv, in, o, (hipStream_t)stream);
}
// ... and HOST arrays: the first device, column batches through the host-entry staging buffer (a column's values do not depend on its
// neighbours, so the results do not depend on the batch size)
int rrtmg_lw_hip_solve(int ncol, int nlay, int cloud, int idrv, const double *plev, const double *emis, const double *tau, const double *fracs,
    const double *planklay, const double *planklev, const double *plankbnd, const double *dplankbnd_dt, const double *cldfr, const double *odcld,
    const unsigned *submask, double *uflx, double *dflx, double *hr, double *uflxc, double *dflxc, double *hrc, double *duflx_dt, double *duflxc_dt)
{
    ENTRY_LOCK;
    if (int rc = check_solve(ncol, nlay, cloud, idrv, {plev, emis, tau, fracs, planklay, planklev, plankbnd, dplankbnd_dt, cldfr, odcld, submask},
                             {uflx, dflx, hr, uflxc, dflxc, hrc, duflx_dt, duflxc_dt})) return rc;
    HIP_TRY(hipDeviceSynchronize());      // asynchronous device-entry work of earlier calls shares the staging
    const size_t n = (size_t)ncol, L = (size_t)nlay;
    const bool dt = idrv == 1, clr = uflxc != nullptr;
    const auto in = [](const double *p, bool on, size_t rows) { return HostIn{on ? p : nullptr, 1, rows, nullptr}; };
    std::vector<HostIn> ins = {in(plev, true, L + 1), in(emis, true, NBND), in(tau, true, L * NGPT), in(fracs, true, L * NGPT), in(planklay, true, L * NBND),
                               in(planklev, true, (L + 1) * NBND), in(plankbnd, true, NBND), in(dplankbnd_dt, dt, NBND), in(cldfr, cloud == 1, L),
                               in(odcld, cloud != 0, L * NBND)};
    // (submask: 32-bit words, MW per column and layer, in 8-byte slots of the staging; copied in by hand below - no host pointer for stage_out)
    const size_t mrows = L * MASK_WORDS;
    std::vector<HostOut> outs = {HostOut{uflx, L + 1, nullptr, true}, HostOut{dflx, L + 1, nullptr, true}, HostOut{hr, L, nullptr, true},
                                 HostOut{uflxc, clr ? L + 1 : 0, nullptr, clr}, HostOut{dflxc, clr ? L + 1 : 0, nullptr, clr}, HostOut{hrc, clr ? L : 0, nullptr, clr},
                                 HostOut{duflx_dt, dt ? L + 1 : 0, nullptr, dt}, HostOut{duflxc_dt, dt ? L + 1 : 0, nullptr, dt},
                                 HostOut{nullptr, cloud == 2 ? (mrows + 1) / 2 : 0, nullptr, false}};
    const int nbmax = balanced_batch(ncol, std::min(eff_batch(nlay), HOST_BATCH));
    if (int rc = stage_alloc(ins, outs, (size_t)nbmax)) return rc;
    hipStream_t s = G.stream.get();
    for (size_t col0 = 0; col0 < n; col0 += (size_t)nbmax) {
        const size_t nb = std::min((size_t)nbmax, n - col0);
        if (int rc = stage_in(ins, n, col0, nb, s)) return rc;
        unsigned *const dmask = cloud == 2 ? reinterpret_cast<unsigned *>(outs[8].d) : nullptr;
        if (dmask) { if (int rc = bounce_h2d_rows(dmask, submask + col0, nb * sizeof(unsigned), n * sizeof(unsigned), mrows)) return rc; }
        const auto od = [&](int k) { return outs[k].active ? outs[k].d : nullptr; };
        if (int rc = solve_launch((int)nb, nlay, (int)nb, (int)nb, cloud, idrv,
                                  {ins[0].d, ins[1].d, ins[2].d, ins[3].d, ins[4].d, ins[5].d, ins[6].d, ins[7].d, ins[8].d, ins[9].d, dmask},
                                  {od(0), od(1), od(2), od(3), od(4), od(5), od(6), od(7)}, s)) return rc;
        if (int rc = stage_out(outs, n, col0, nb, s)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int rrtmg_lw_hip_gas_optics_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, int idrv, GCM_PARAMS_AS,
    void *taug, void *fracs, void *planklay, void *planklev, void *plankbnd, void *dplankbnd_dt, void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    if (plain) return gas_optics_device_ld(ncol, nlay, idrv, GCM_NAMES_AS, (double *)taug, (double *)fracs, (double *)planklay, (double *)planklev,
                                           (double *)plankbnd, (double *)dplankbnd_dt, ld, stream);
    return gas_optics_device_as(f, ncol, nlay, idrv, {GCM_NAMES_AS},
                                OptOut{(double *)taug, (double *)fracs, (double *)planklay, (double *)planklev, (double *)plankbnd, (double *)dplankbnd_dt}, stream, ld);
}

int rrtmg_lw_hip_adjust_tsfc_device_view(const rrtmg_lw_hip_array_view *view, int ncol, int nlay, const void *plev, const void *dtsfc,
    const void *uflx, const void *dflx, const void *duflx_dt, const void *uflxc, const void *dflxc, const void *duflxc_dt,
    void *uflx_adj, void *hr_adj, void *uflxc_adj, void *hrc_adj, void *stream)
{
    rrtmg_lw_hip_array_form f;
    int ld = 0;
    bool plain = false;
    if (int rc = view_check(view, ncol, &f, &ld, &plain)) return rc;
    return adjust_device(f, ncol, nlay, {plev, dtsfc, uflx, dflx, duflx_dt, uflxc, dflxc, duflxc_dt}, {uflx_adj, hr_adj, uflxc_adj, hrc_adj}, stream, ld);
}

}  // extern "C"
