// common.h -- internal declarations shared by the HIP translation units of libsvhip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "pcg64.h"
#include "supervillain_amd.h"

// Allocation log (diagnostics): with SV_ALLOC_LOG set, every device / pinned allocation and free the library makes
// is written to stderr with its address range and call site, so that the faulting virtual address a GPU memory fault
// reports (AMD_LOG_LEVEL=1) can be matched to the buffer -- live or already freed -- it belongs to.  Off: one
// cached flag test per call.
#define SV_HIDDEN __attribute__((visibility("hidden")))
SV_HIDDEN hipError_t sv_log_malloc(void **p, size_t bytes, const char *site);
SV_HIDDEN hipError_t sv_log_free(void *p, const char *site);
SV_HIDDEN hipError_t sv_log_host_malloc(void **p, size_t bytes, unsigned flags, const char *site);
SV_HIDDEN hipError_t sv_log_host_free(void *p, const char *site);
#define SV_STR2(x) #x
#define SV_STR(x) SV_STR2(x)
#define hipMalloc(p, n) sv_log_malloc((void **)(p), (n), __FILE__ ":" SV_STR(__LINE__))
#define hipFree(p) sv_log_free((void *)(p), __FILE__ ":" SV_STR(__LINE__))
#define hipHostMalloc(p, n, f) sv_log_host_malloc((void **)(p), (n), (f), __FILE__ ":" SV_STR(__LINE__))
#define hipHostFree(p) sv_log_host_free((void *)(p), __FILE__ ":" SV_STR(__LINE__))

namespace sv {

// ----------------------------------------------------------------------------------------------
// RNG blocks.  A sweep consumes the NumPy stream as a fixed sequence of blocks:
// uniform blocks (one u64 per draw) and bounded blocks (one uint32 per draw through NumPy's
// buffered Lemire sampler, plus one extra uint32 per rejection).  The host planner walks a cursor
// through the blocks; kernels address any draw of a block by position.
struct Block {
    uint64_t base_lo, base_hi;  // state whose XSL-RR output is this block's u64 #0
    uint32_t has, buf;          // bounded: a buffered half-word precedes the u64 stream
    int32_t nskip, skip0;       // bounded: rejected stream positions are skips[skip0 .. skip0+nskip)
};

struct Cursor {
    u128 s;  // state BEFORE the next draw
    uint32_t has, buf;
};

enum BlockKind { UNIFORM = 0, BOUNDED = 1 };

struct BlockSpec {
    BlockKind kind;
    uint32_t count;  // draws
};

// Host PCG64 helpers
u128 host_jump(u128 s, u128 inc, uint64_t steps);
Affine host_power(u128 inc, uint64_t steps);  // the map of `steps` PCG64 steps
uint64_t host_output_at(u128 s, u128 inc, uint64_t pos);  // X_pos after state s (X_0 = output of one step)

// Plan one block starting at `cur`; advances `cur`.  `skips` is the sorted list of rejected
// stream positions known for this block (bounded only).
Block plan_block(Cursor &cur, u128 inc, const BlockSpec &spec, const std::vector<uint32_t> &skips, int32_t skip0);

// Device jump tables for one increment (cached in the context).
JumpTables make_tables(u128 inc);

// Rejection report written by kernels: the sweep (within the launch batch), block and stream position.
struct Report {
    uint32_t sweep, block, pos, pad;
};
static constexpr int MAX_REPORTS = 1024;
// reports copied with a batch's tail (sv_ctx: d_abort, d_nreport and d_reports are one allocation, 16 B apart)
static constexpr int TAIL_REPORTS = 15;

// Device-side per-call scratch: abort flag, reports, stats accumulators.
struct DevScratch {
    int32_t *abort;     // nonzero: a rejection (or overflow) was met; later sweeps exit immediately
    uint32_t *nreport;  // count of reports
    Report *reports;
    int32_t *hflag = nullptr;  // optional host-mapped copy of the abort flag (the host polls it between chunks)
    // optional (replica batches): the first sweep with a report (atomic min; INT32_MAX when none).  With a gate,
    // launches exit only behind a sweep that reported, so the failing sweep itself completes for every replica
    // and only the replicas that reported in it are replayed
    int32_t *gate = nullptr;
};

// Asynchronous emission of a resident state: the state is snapshotted on the compute
// stream (device copy, stream-ordered after every queued sweep) into one of two emission buffers, and the
// buffer goes to the host on a copy stream of its own, overlapping the sweeps that follow.  Before a buffer
// is reused the compute stream waits (on the device) for its previous copy.
struct Emitter {
    hipStream_t copy = nullptr;
    void *buf[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    size_t bytes[2] = {0, 0};  // per field
    hipEvent_t snap[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    int k = 0;
    int device = 0;
    // copy fields (a: bytes0, b: bytes1, either may be null) of the state to the host arrays ha, hb
    void emit(hipStream_t compute, const void *a, size_t bytes0, const void *b, size_t bytes1, void *ha, void *hb);
    void wait();     // every emission has reached the host
    hipError_t release();  // drains the copy stream, frees the buffers; the drain's result
};

}  // namespace sv

// ----------------------------------------------------------------------------------------------
// Context and device-resident states (opaque in the C-ABI).
struct sv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::pair<uint64_t, uint64_t>, sv::JumpTables *> tables;  // per PCG64 increment (device, 40 KB each)
    static constexpr size_t MAX_TABLES = 1024;                         // 40 MB of HBM before the cache is dropped
    int64_t table_purges = 0;
    size_t table_cap = 0;  // sv_ctx_set_table_cap (tests): a smaller cache for this context; 0 = the default
    // scratch
    int32_t *d_abort = nullptr;
    uint32_t *d_nreport = nullptr;
    sv::Report *d_reports = nullptr;
    sv::Block *d_blocks = nullptr;
    size_t blocks_cap = 0;
    uint32_t *d_skips = nullptr;
    size_t skips_cap = 0;
    sv_stats *d_stats = nullptr;
    size_t stats_cap = 0;
    // pinned host image of d_abort: batches that cannot meet a rejection copy it with their stats (one sync)
    int32_t *h_abort = nullptr;
    // host-mapped abort flag (fine-grained pinned memory: h_flag for the host, d_flag for kernels), written by a
    // kernel's rejection report so that the host can stop enqueueing a batch that has failed (run_fused)
    int32_t *h_flag = nullptr, *d_flag = nullptr;
    int32_t *h_prog = nullptr, *d_prog = nullptr;  // the next word: batch launches started (FArgs::progress)
    // pinned batch tail (abort flag, report count, statistics) of the single-lattice Villain run: one sync
    char *h_tail = nullptr;
    size_t tail_cap = 0;
    // optional per-launch timing of the sweep kernels (hipEvents on ctx->stream)
    bool timing = false;
    int timing_mode = 0;  // 1: events around each batch of launches, 2: around every launch
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
    std::vector<int64_t> ev_launches;
    std::vector<int64_t> ev_first;  // index of the segment's first launch within its batch
    double timed_ms = 0.0;
    int64_t timed_launches = 0;
    // Villain NeighborhoodUpdate sweeps by kernel (sv_ctx_sweep_counts): villain_sweep_hot (+ _fr), the general
    // fused kernel (villain_sweep_fused: int32 n image, skip lists), the per-colour int64 path (villain_pass_generic)
    int64_t sweeps_hot = 0, sweeps_fused = 0, sweeps_generic = 0;
    int64_t sweeps_split = 0;  // replays of rejected sweeps on villain_sweep_hot_split (sv_ctx_split_counts)
    // of the hot sweeps: those run by multi-sweep band launches, and the launches (sv_ctx_band_counts)
    int64_t sweeps_band = 0, launches_band = 0;
    // the same for temporal-blocking launches (sv_ctx_block_counts), and the multi-sweep mode (sv_ctx_set_multisweep:
    // 0 blocks or bands, 1 blocks only, 2 bands only, 3 one sweep per launch)
    int64_t sweeps_block = 0, launches_block = 0;
    int32_t multisweep = 0, block_k = 0;  // (block_k: sweeps per temporal-blocking launch, 0 = the default)
    void time_begin(hipEvent_t *a);
    void time_end(hipEvent_t a, int64_t launches = 1, int64_t first = 0);
    void time_collect();  // after a stream sync
    void time_discard();  // drop pending (unsynchronized-safe: after a stream sync)
    void time_keep_before(int64_t bad);  // an aborted batch: keep the segments that ended before launch `bad`

    // deferred statistics (sv_ctx_set_deferred): a run whose sweeps cannot meet a NumPy Lemire rejection leaves
    // its statistics (and abort flag) in a pinned staging area and returns without synchronizing; sv_ctx_sync
    // lands them in the caller's arrays.  One synchronization per device-resident program step instead of one
    // per member generator.
    struct Landing {
        sv_stats *dst;
        size_t off;
        int64_t count;
        size_t abort_slot;
    };
    bool deferred = false;
    sv_stats *h_stage = nullptr;
    int32_t *h_stage_abort = nullptr;
    size_t stage_cap = 0, stage_used = 0, abort_cap = 0, abort_used = 0;
    std::vector<Landing> landings;
    bool defer_stats(sv_stats *dst, int64_t count);  // queued (deferred mode) or false: the caller synchronizes
    void land();                                      // after a stream synchronization

    const sv::JumpTables *jump_tables(uint64_t inc_hi, uint64_t inc_lo);
    void ensure_blocks(size_t n);
    void ensure_skips(size_t n);
    void ensure_stats(size_t n);
    // a batch plan (descriptors, skip positions) to d_blocks / d_skips through pinned staging: two pinned buffers
    // used in turn (an upload reuses the one of two uploads before, across the batch's synchronization), so the
    // copies are plain asynchronous DMA instead of pageable staging (~20 us of host time each)
    // (offset: the descriptors go to d_blocks + offset -- the second part of a two-part plan, whose capacity the first
    // part ensured, so that d_blocks does not move under launches already enqueued)
    void upload_plan(const sv::Block *blocks, size_t nblocks, const uint32_t *skips, size_t nskips, size_t offset = 0);
    char *h_plan[2] = {nullptr, nullptr};
    size_t h_plan_cap[2] = {0, 0};
    hipEvent_t ev_plan[2] = {nullptr, nullptr};  // recorded after each buffer's copies (deferred runs do not sync)
    int h_plan_i = 0;
};

struct sv_villain {
    sv_ctx *ctx = nullptr;
    int32_t N = 0;
    double *phi[2] = {nullptr, nullptr};  // ping-pong (fused sweep reads one, writes the other)
    int64_t *n[2] = {nullptr, nullptr};
    int cur = 0;
    double *r = nullptr;        // generic path: residual r = d(phi) - 2 pi n, kept incrementally
    double *snap_phi = nullptr;  // generic path snapshot
    int64_t *snap_n = nullptr;
    int32_t *sites = nullptr;    // generic path: colour site lists (row-major), concatenated
    int32_t ncol = 0;
    int64_t count[4] = {0, 0, 0, 0};
    int64_t offset[4] = {0, 0, 0, 0};
    sv::Emitter emitter;
    std::vector<int64_t> partial;  // host scratch
    char *d_aux = nullptr;         // small per-call device block (CohomologyUpdate: rng | stats | plan)
    char *h_aux = nullptr;         // its pinned host image
    size_t aux_cap = 0;
    unsigned long long *d_obs = nullptr;  // inline observables: the OBS_WORDS exact words (coarse-grained hipMalloc)
    unsigned long long *h_obs = nullptr;  // and their pinned host image
    int32_t *d_strips = nullptr;   // villain_sweep_hot's strip table (strip_schedule), n_strips entries of 3
    int32_t n_strips = 0;
    std::vector<int32_t> h_strips;  // (its host copy: the split replay orders its straddling strips first)
    std::string strips_key;        // the schedule the table holds
    // multi-sweep band launches (villain_sweep_hot_band): the launch's scratch buffers (sweep outputs 1..K-1) and
    // the per-XCD ticket / barrier counters followed by the batch's gate word
    std::vector<double *> band_phi;
    std::vector<int64_t *> band_n;
    uint32_t *band_ctrl = nullptr;
};

namespace sv {
// worm.hip: Villain worms over R chains stored (R, N, N) phi / (R, 2, N, N) n on the device
void villain_worms_device(sv_ctx *ctx, int32_t R, int32_t N, const double *phi, int64_t *n, double kappa, int64_t W,
                          int32_t worms, int64_t max_moves, sv_rng *rngs, int64_t *hist, int64_t *lengths);
void worm_release(sv_ctx *ctx);  // frees the context's worm scratch (sv_ctx_destroy)
void correlators_release(sv_ctx *ctx);  // correlators.hip: frees the context's correlator work buffers (sv_ctx_destroy)
}  // namespace sv

struct sv_worldline {
    sv_ctx *ctx = nullptr;
    int32_t N = 0;
    int32_t v_is_float = 0;
    int64_t *m = nullptr;
    void *v = nullptr;  // int64 or double (N*N)
    int64_t *snap_m = nullptr;
    void *snap_v = nullptr;
    double *f = nullptr;         // sequential plaquette: f = m - delta(v)/W kept incrementally
    int32_t *order = nullptr;    // sequential plaquette: plaquettes grouped by dependency level
    int32_t *pos = nullptr;      // sequential plaquette: visit position of each plaquette
    int32_t *lev = nullptr;      // sequential plaquette: dependency level of each plaquette
    int64_t *ord64 = nullptr;    // sequential plaquette: the caller's visit order, on the device
    int32_t *lcnt = nullptr;     // sequential plaquette: per-level counts / slots, then LFLAGS flags
    uint32_t *h_perm[2] = {nullptr, nullptr};  // reference-order runs: pinned visit orders (the native permutations)
    void *stripes = nullptr;     // striped per-sweep statistics (worldline.hip StatStripe[64][16])
    sv::Emitter emitter;
    int32_t *sites = nullptr;
    int32_t ncol = 0;
    int64_t count[4] = {0, 0, 0, 0};
    int64_t offset[4] = {0, 0, 0, 0};
    char *d_aux = nullptr;  // WrappingUpdate scratch (cycle proposals, dS, flags, pairwise plan)
    size_t aux_cap = 0;
    // worldline_fused.hip reads (m, v) and writes the other buffer pair; the pointers swap per fused step
    int64_t *m_alt = nullptr;
    void *v_alt = nullptr;
    int64_t *m_at_snap = nullptr;  // the (m, v) pointers a snapshot was taken from (restore puts them back)
    void *v_at_snap = nullptr;
    bool wf_off = false;           // |m| or |v| outgrew the fused kernel's int32 image: four-pass kernels only
};

#define SV_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            throw std::runtime_error(std::string(#call) + " failed: " + hipGetErrorString(e_));       \
    } while (0)

// SV_SYNC_CHECK=1 in the environment (read once per process): after every kernel launch the launch error is read and
// the launch's stream synchronized, and a failure throws naming the kernel -- so a fault (an illegal address, an
// abort) is attributed to the launch that caused it instead of surfacing at a later copy or synchronization.  Every
// launch site is written `kernel<<<...>>>(args), SV_LAUNCHED("kernel", stream);` (one expression statement).  Off by
// default: one flag test per launch.  (VERDICT r5 next #6.)
namespace sv {
inline bool sync_check_on() {
    static const bool on = [] {
        const char *e = std::getenv("SV_SYNC_CHECK");
        return e && e[0] && e[0] != '0';
    }();
    return on;
}
[[noreturn]] void launch_failed(const char *kernel, const char *stage, hipError_t e);  // capi.hip: throws
inline void launch_check(const char *kernel, hipStream_t s) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) launch_failed(kernel, "launch", e);
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) launch_failed(kernel, "execution", e);
}
}  // namespace sv
#define SV_LAUNCHED(kernel, stream) (sv::sync_check_on() ? sv::launch_check(kernel, stream) : (void)0)

// Exact Metropolis acceptance sums (the float statistics must not depend on the launch geometry).
// A proposal's acceptance probability p in [0, 1] enters as the integer round(p 2^51): x = p + 2.0 lies in the binade
// [2, 4) (ulp 2^-51), so bits(x) = 0x4000000000000000 + round(p 2^51) (round to nearest even).  A lane adds the raw bits
// modulo 2^64 (fx_add: one f64 add and one 64-bit integer add per proposal); after k < 2^11 terms the low 62 bits are
// the exact sum of its k values (the k 2^62 of the exponents only touch bits 62 and 63).  It flushes that sum, scaled to
// T = sum 2^52 (the 2^-103 grid the three-limb words use), as three 38-bit limbs, so every later addition -- over lanes,
// waves, workgroups, strips, tiles, replica batches, launches -- is an integer addition whose result does not depend on
// its order, and the statistic is fx_value(limb sums) = T 2^-103: the same double whatever the strip heights, layouts,
// tile grids or replica counts of the run.  Resolution: 2^-52 per proposal, absolute (the sweep's sum is within
// 2^-52 x proposals of the exact sum of the p: relative 1e-15 at any acceptance rate above 0.1%).  The oracle keeps
// the 2^-103 grid (oracle/sv_oracle.c fx_term_limbs), within rounding of the reference's pairwise sums at any rate; a
// second, 2^-103 level here measured 1.5% on the headline sweep and 5% on config 3 (r6) and is not kept.
// On the device a stats slot holds the three limb sums in its host-owned fields until it is finalized (stats_finalize,
// or fx_value on the host for the domain summaries): proposed = limb 0, rejections = limb 1, acceptance_sum's bits =
// limb 2.
namespace sv {
constexpr uint64_t FX_LANE_MASK = (uint64_t(1) << 62) - 1, FX_LIMB = (uint64_t(1) << 38) - 1;
struct AccFx {
    uint64_t a = 0;  // raw bits of p + 2.0, summed mod 2^64
};
__device__ __forceinline__ void fx_add(AccFx &s, double p) { s.a += (uint64_t)__double_as_longlong(p + 2.0); }
// a lane's exact value sum T = (a mod 2^62) 2^52 (< 2^114) as three 38-bit limbs
__device__ __forceinline__ void fx_limbs(const AccFx &s, unsigned long long &w0, unsigned long long &w1,
                                         unsigned long long &w2) {
    const unsigned __int128 T = (unsigned __int128)(s.a & FX_LANE_MASK) << 52;
    w0 = (uint64_t)T & FX_LIMB;
    w1 = (uint64_t)(T >> 38) & FX_LIMB;
    w2 = (uint64_t)(T >> 76);
}
// device word i of a stats slot: 0 accepted, 1..3 the acceptance limbs (proposed, rejections, acceptance_sum's bits)
__device__ __forceinline__ unsigned long long *stat_word(sv_stats *st, int i) {
    return i == 0 ? (unsigned long long *)&st->accepted
         : i == 1 ? (unsigned long long *)&st->proposed
         : i == 2 ? (unsigned long long *)&st->rejections
                  : (unsigned long long *)&st->acceptance_sum;
}
__host__ __device__ __forceinline__ uint64_t stat_limb(const sv_stats &st, int i) {  // i = 0, 1, 2
    if (i == 0) return (uint64_t)st.proposed;
    if (i == 1) return (uint64_t)st.rejections;
    uint64_t w;
    memcpy(&w, &st.acceptance_sum, sizeof w);
    return w;
}
// the statistic from the three limb sums (each < 2^64): a deterministic function of the exact total T 2^-103
__host__ __device__ __forceinline__ double fx_value(uint64_t w0, uint64_t w1, uint64_t w2) {
    w1 += w0 >> 38;
    w0 &= FX_LIMB;
    w2 += w1 >> 38;
    w1 &= FX_LIMB;
    return ((double)w2 * 0x1p76 + (double)w1 * 0x1p38 + (double)w0) * 0x1p-103;
}

// Exact inline observables (same reason).  A site's action term t = l0^2 + l1^2 (l the link residuals, in the
// reference's operation order) enters as round(t 2^40) when t < 2^12 (|l| < 45; at kappa >= 0.05 a larger residual
// has Boltzmann weight below e^-100), else as a double added to the big-term word in arrival order -- the one case
// whose sum still depends on the launch geometry.  The resolution is 2^-41 per site (an absolute error below 2^-41 V
// on the action sum: relative 1e-13 or less in any state whose mean t exceeds 0.005).  A lane holds at most 256 such
// values (< 2^60) and flushes them as 32-bit halves (lo, hi).  The integer observables (sum dn^2, sum n0, sum n1) are
// integer sums.
// Per (replica, sweep) the OBS_WORDS words are: the action (lo, hi), sum dn^2, sum n0, sum n1 (two's complement),
// the big-term double; obs_raw() turns them into the 4 raw sums of the C-ABI {sum l^2, sum dn^2, sum n0, sum n1}.
constexpr int OBS_WORDS = 6;
constexpr double ACT_LIMIT = 4096.0;
__device__ __forceinline__ uint64_t act_fx(double t) {  // t in [0, ACT_LIMIT)
    // t 2^40 + 2^52 rounded once (t 2^40 is exact): the double's low bits are round(t 2^40)
    return (uint64_t)__double_as_longlong(__builtin_fma(t, 0x1p40, 0x1p52)) - 0x4330000000000000ull;
}
__host__ __device__ __forceinline__ double act_value(uint64_t lo, uint64_t hi) {
    const uint64_t h = hi + (lo >> 32), l = lo & 0xffffffffull;
    return ((double)h * 4294967296.0 + (double)l) * 0x1p-40;
}
inline void obs_raw(const unsigned long long *w, double *raw) {
    double big;
    std::memcpy(&big, &w[5], sizeof big);
    raw[0] = act_value(w[0], w[1]) + big;
    raw[1] = (double)w[2];
    raw[2] = (double)(int64_t)w[3];
    raw[3] = (double)(int64_t)w[4];
}
}  // namespace sv
namespace svh {
// the exact acceptance limbs of n device stats slots -> their acceptance_sum (villain.hip); enqueued before every copy
// of device statistics to the host (a finalized slot is marked and left alone by a second finalize)
void finalize_stats(sv_stats *d, int64_t n, hipStream_t stream);
}  // namespace svh

// The drain at the start of every sv_*_destroy: the work queued on the context stream (and on `side`, an object's
// own stream) ends before anything is freed.  A failure there is the failure of work queued earlier -- by this
// object or by a call before it -- so it is recorded in the context's error (sv_last_error) with the object's name
// instead of being discarded, and the destroy still frees everything and returns -2 (the Python wrappers warn).
inline int sv_destroy_drain(sv_ctx *ctx, const char *what, hipStream_t side = nullptr) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (side) {
        const hipError_t e2 = hipStreamSynchronize(side);
        if (e == hipSuccess) e = e2;
    }
    if (e == hipSuccess) return 0;
    ctx->err = std::string(what) + ": work queued before it was destroyed failed: " + hipGetErrorString(e);
    return -2;
}

namespace sv {
// mt19937.hip: np.random.permutation(n) of NumPy's legacy global RandomState as 32-bit indices, advancing (key, pos)
void legacy_permutation32(uint32_t *key, int32_t &pos, int64_t n, uint32_t *out);
void legacy_intervals(uint32_t *key, int32_t &pos, int64_t n, uint32_t *j);  // its two stages: the draws (serial)
void shuffle_from_intervals(const uint32_t *j, int64_t n, uint32_t *out);    // and the swaps
// colour lists for D=2 (compact.py:191-239); returns ncol, fills site lists in row-major order
int build_colors(int32_t N, std::vector<int32_t> &sites, int64_t count[4], int64_t offset[4]);
}  // namespace sv
