// ngp_api.hip -- C ABI of libnextgp_hip.so (include/nextgp_hip.h): handle lifecycle, panel
// upload / generation with re-tiling, model set-up, the per-iteration launch sequence of the
// blocked Gibbs sweep, state and posterior read-back.  gfx950 only; there is NO CPU fallback:
// without a usable device every entry point fails with NGP_ERR_NODEVICE / NGP_ERR_HIP.
#include <hip/hip_runtime.h>
#include <cassert>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <array>
#include <atomic>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nextgp_hip.h"
#include "ngp_kernels.h"
#include "ngp_random.h"
#include "ngp_fixed_sparse.h"
#include "ngp_random_tuple.h"
#include "ngp_dense.h"
#include "ngp_hybrid.h"
#include "ngp_logvar.h"
#include "ngp_predict.h"
#include "ngp_bed.h"
#include "ngp_holdout.h"
#include "ngp_liability.h"
#include "ngp_threshold.h"
#include "ngp_genvar.h"
#include "ngp_diag.h"
#include "ngp_sweep_args.h"
#include "ngp_state.h"

using namespace ngp;

namespace {

// Owning device array: move-only, the destructor frees it.  alloc() (zeroed) and alloc_raw() (not zeroed: staging buffers, sample
// ring slots, all-reduce buffers) free the old array first.  Reads as a T * wherever a launch or a copy takes one.  This type and
// PinnedArray are the only code of this file that allocates or frees device or pinned host memory.
template <typename T>
struct DevArray {
    T *p = nullptr;
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    DevArray(DevArray &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevArray &operator=(DevArray &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DevArray() { reset(); }
    void reset() { if (p) { (void)hipFree(p); p = nullptr; } }
    hipError_t alloc_raw(size_t n) { reset(); const hipError_t e = hipMalloc((void **)&p, n * sizeof(T)); if (e != hipSuccess) p = nullptr; return e; }
    int alloc(ngp_handle *h, size_t n);  // n (at least 1) zeroed entries on h's stream; NGP_ERR_NOMEM / NGP_ERR_HIP through fail() (below)
    T *get() const { return p; }
    operator T *() const { return p; }
};

// Owning pinned host array (hipHostMalloc): the counterpart of DevArray for staging through the host
template <typename T>
struct PinnedArray {
    T *p = nullptr;
    PinnedArray() = default;
    PinnedArray(const PinnedArray &) = delete;
    PinnedArray &operator=(const PinnedArray &) = delete;
    PinnedArray(PinnedArray &&o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedArray &operator=(PinnedArray &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~PinnedArray() { reset(); }
    void reset() { if (p) { (void)hipHostFree(p); p = nullptr; } }
    hipError_t alloc_raw(size_t n) { reset(); const hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault); if (e != hipSuccess) p = nullptr; return e; }
    T *get() const { return p; }
    operator T *() const { return p; }
};

struct FileCloser {
    void operator()(FILE *f) const { std::fclose(f); }
};
using File = std::unique_ptr<FILE, FileCloser>;  // a FILE * closed when it goes out of scope (release() it to check fclose)

struct HFix {  // one fixed-effect set beyond the intercept
    int64_t ncol = 0, off = 0;
    DevArray<double> d_X, d_xpx0, d_xpxR, d_lhs0, d_rhs0;
    // a set given as a sparse matrix (ngp_add_fixed_set_sparse; kernels in ngp_fixed_sparse.h) holds none of the above, but:
    bool sparse = false;
    DevArray<long long> d_cptr, d_rptr, d_xptr;  // X by columns (CSC) and by records (CSR); X'X by rows (CSR, columns ascending)
    DevArray<int> d_crow, d_rcol, d_xcol;
    DevArray<double> d_cval, d_rval, d_xval;     // (d_xval: the unridged X'X; the ridge changes its diagonal only)
    DevArray<double> d_diagR, d_scr;             // the ridged diagonal; NGP_FS_ROWS x ncol scratch
    struct Launch { int wide; int d0, d1; long long r0, r1; };  // wide: the columns order[r0 .. r1) of depth d0; else the depths d0 .. d1 - 1 in one workgroup
    DevArray<int> d_order;                       // the columns by (depth, column)
    DevArray<long long> d_dptr;
    std::vector<Launch> plan;
};

// A dense q x q precision on the device (ngp_add_random_set_dense): row l at K + l ld.  Read-only once a set uses it; sets of several
// handles (chains) may hold the same matrix, which lives as long as any of them.
struct DenseK {
    DevArray<double> K;
    int64_t q = 0, ld = 0;
    uint64_t digest = 0;  // of all q x q entries (dense_digest, once, when a set first takes the matrix): the model signature of snapshots
};

// The genomic relationship matrix under construction (ngp_grm_begin .. ngp_grm_invert): column-major with leading dimension ld = N
// rounded up to 64, rows and columns beyond N zero.  state: 1 columns may arrive, 2 G complete (ngp_grm_end), 3 inverted, 4 the corner
// block D = G_w^-1 - A22^-1 of single-step GBLUP (ngp_grm_single_step).
struct Grm {
    std::shared_ptr<DenseK> m;
    int state = 0, method = 1;
    int64_t N = 0, ncols = 0;
    double sum2pq = 0.0;  // method 1: sum of 2 p q over the columns so far, in column order
};

struct HRand {  // one (1|g) random-effect set (src/mme.jl:165-272), sampled after the fixed-effect sets (src/samplers.jl:43-46)
    int64_t q = 0;
    int tk = 1;                // components: 1, or the k of a correlated (Tuple) set (ngp_add_random_set_tuple; kernels in ngp_random_tuple.h)
    double df = 0.0, scale = 0.0, varU0 = 0.0;
    double sdf = 0.0;          // tk = 1: scale * df (k_rand_var), the product formed once on the host
    std::vector<double> scaleM, varU0M;  // tk x tk, row-major (tk = 1: sdf and varU0)
    bool offdiag = false;      // K has entries off its diagonal: Gauss-Seidel (k_rand_gs); otherwise every level is drawn on its own
    uint64_t fine_calls = 0;   // ngp_sample_random_set calls (their iteration key, as ngp_sweep_set's)
    DevArray<long long> d_lptr, d_kptr;  // records of level l: d_lrows[d_lptr[l] .. d_lptr[l + 1]); CSR of K
    DevArray<int> d_lrows, d_level, d_kcol;
    DevArray<double> d_kval, d_kdiag, d_zpz;
    DevArray<double> d_u, d_sum_u;  // q x tk, the components of a level adjacent
    DevArray<double> d_vu;     // [varU, sum_varU], tk x tk each
    DevArray<double> d_scr;    // NGP_RS_ROWS x q scratch (ngp_random.h); a tuple set: tup_scr_len doubles (ngp_random_tuple.h)
    // a tuple set (tk > 1): d_lptr / d_lrows / d_level per component; the W blocks of the header: diagonal ones dense, the others CSR
    DevArray<long long> d_wptr;
    DevArray<int> d_wcol;
    DevArray<double> d_wd, d_wval, d_scaleM;
    uint64_t sig = 0;          // digest of the level coding and K (snapshots refuse another random-effect model)
    std::shared_ptr<DenseK> dk;  // a dense K (ngp_add_random_set_dense): the blocked engine of ngp_dense.h instead of k_rand_gs / k_rand_var
    // a hybrid set (ngp_add_random_set_hybrid, ngp_hybrid.h): the CSR holds S without its trailing x trailing entries, dk the nd x nd block
    // T = D + S_tt over the levels hd .. q - 1; the level schedule covers the head rows 0 .. hd - 1
    bool hyb = false;
    int64_t hd = 0;
    // the level schedule of a CSR K with off-diagonal entries (ngp_random.h, k_rand_sched_*): rows sorted by (depth, row), and the launches
    struct Launch { int wide; int d0, d1; long long r0, r1; };  // wide: the rows order[r0 .. r1) of depth d0; else the depths d0 .. d1 - 1 in one workgroup
    DevArray<int> d_order;
    DevArray<long long> d_dptr;
    std::vector<Launch> plan;
    int64_t ndepth = 0;
    int sched_mode = 0;        // ngp_set_random_schedule: 0 automatic, 1 serial (k_rand_gs), 2 scheduled
    bool scheduled() const { return sched_mode == 2 || (sched_mode == 0 && (hyb ? hd : q) > NGP_RS_AUTO_LEVELS_PER_DEPTH * ndepth); }
};
// q of a set as the sample file's header and the snapshot signature carry it: q, and k - 1 of a tuple set in the bits from 32 up
// (q < 2^31; a set of one component writes the word it always wrote)
inline int64_t rand_q_word(const HRand &R) { return R.q | ((int64_t)(R.tk - 1) << 32); }

struct HLv {  // the variance model of one BayesLV marker set (src/mme.jl:418-439; kernels and state layout in ngp_logvar.h)
    int set = -1;              // its marker set
    int64_t n = 0;             // loci
    int ncov = 0, mode = 0;    // covariate columns; 0: varZeta fixed, 1: var(zeta), 2: frac * var(logVar)
    double frac = 0.0, varZeta0 = 0.0;
    std::vector<double> zeta0; // starting values given by the caller (empty: keyed uniforms, k_lv_start)
    DevArray<double> d_C, d_iCpC, d_zeta, d_logv, d_part, d_vpart;
    DevArray<double> d_st;     // NGP_LV_WORDS doubles: c | varZeta | their posterior sums | trapped | mean
    DevArray<int> d_trapseg;
};

struct HRc {  // the per-locus state of one BayesRCpi marker set (src/mme.jl:384-403; kernels in ngp_bayesrc.h)
    int set = -1;              // its marker set
    int A = 0, Kc = 0;         // annotations, classes
    int64_t n = 0, nseg = 0;   // loci, 256-locus segments
    std::vector<uint8_t> mask; // bit a: the locus has annotation a (annotInput)
    DevArray<uint8_t> d_mask, d_cat;
    DevArray<double> d_prob, d_sum, d_part;  // annotProb [A][n], sum_annot [A][n], segment partials [nseg][A]
    DevArray<int> d_cnt;       // [nseg][NGP_RMAX]
    DRc dev() { DRc R; R.prob = d_prob; R.mask = d_mask; R.cat = d_cat; R.sum = d_sum; R.part = d_part; R.cnt = d_cnt; R.nseg = nseg; return R; }
};

// The prediction panel beside a training panel (ngp_begin_prediction_panel): Np individuals x the training panel's columns, in the
// training tile layout with a plan of its own -- S shards of R <= NGP_PRED_MAXR rows
struct PredPanel {
    DevArray<float> tiles;  // fp32 tiles, or (compact storage) one byte per element behind the same pointer
    DevArray<double> mean;  // Ppad: what was subtracted from every column (the training mean where the caller asked for centring, else 0)
    int64_t Np = 0, R = 0, S = 0;
    uint64_t id = 0;        // unique per panel: what a chain remembers of the panel its sums belong to
    bool done = false;      // ngp_end_prediction_panel has run: the kept iterations of every chain on the panel now predict
};

// The arrays of one uploaded panel: the handles that share it (ngp_share_panel) hold a std::shared_ptr each
struct PanelMem {
    std::shared_ptr<PredPanel> pred;  // null: no prediction panel
    DevArray<float> tiles;  // fp32 tiles, or (compact storage) one byte per element behind the same pointer
    DevArray<double> mean;  // column means, Ppad
    DevArray<double> gramx, mpm;  // Gram window (D planes per block), x'x
    double mpm_max = 0.0;   // max_j x_j'x_j of the panel (scale of the accumulators, k_head)
};

// Kept samples streamed to a binary file while the chain runs (ngp_set_sample_file): a ring of NSLOT records on the device, copied to
// pinned host memory on a second stream, written by a thread of its own.  The chain's stream never waits for the file -- only for a
// ring slot, when the writer is NSLOT samples behind.
struct SampleStream {
    static constexpr int NSLOT = 4;
    File f;
    std::string path;
    size_t rec_bytes = 0;
    bool header_written = false;
    int device = 0;
    DevArray<unsigned char> d_slot[NSLOT];
    PinnedArray<unsigned char> h_slot[NSLOT];
    hipEvent_t ev_packed[NSLOT] = {nullptr, nullptr, nullptr, nullptr}, ev_copied[NSLOT] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    std::thread writer;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<int> queue;          // slots whose copy has been enqueued, in order
    bool busy[NSLOT] = {false, false, false, false};
    bool stop = false, io_error = false;
    int64_t nenq = 0, nwritten = 0, ndropped = 0;
    ~SampleStream();  // (below) joins the writer before the slots are freed
};

struct HSet {
    int64_t col0, ncol;
    int method;
    double df, scale;
    int64_t nreg;
    int64_t vb_off;
    int estPi;
    uint64_t fine_calls;
    double pi0;               // prior inclusion probability (src/mme.jl:351,360): what ngp_set_y goes back to
    std::vector<double> vb0;  // initial variances (src/mme.jl:516)
    int K = 0;                // BayesR: classes, their multipliers and prior probabilities (src/mme.jl:374-383)
    std::vector<double> vcls, rpi;
    int tk = 0;               // Tuple (correlated BayesPR) set: number of correlated sets; nreg k x k variance matrices in varBeta
    int64_t nloc = 0;
    int lv = -1;              // BayesLV set: its entry of ModelMem::lv (the device's DSet says BayesPR: the sweep is BayesPR's)
    int rc = -1;              // BayesRCpi set: its entry of ModelMem::rc; K then counts its A * Kc slots, vcls / rpi are indexed by the slot
};

std::string g_create_err;

/* ---- the plan of the persistent sweep: how a panel is swept, decided in one place ---------------------------------------- */

// what the caller asked for before the panel was set (ngp_configure, ngp_set_storage, ngp_set_near_lags, ngp_set_max_shards,
// ngp_set_streamer)
struct PlanRequest {
    int storage = 0;       // 0: centred fp32 tiles; 1: compact -- byte tiles + Float64 column means (ngp_set_storage)
    int mode = 1;          // 1: persistent sweep kernel, 0: one streaming + one recursion launch per block
    int lag = 8;           // look-ahead D of the persistent sweep (blocks); shards taller than 128 rows are capped at 5
    bool lag_auto = true;  // lag not chosen by the caller (ngp_configure): tall shards then take the measured best
    int near_req = 0;      // near lags requested (0 = automatic)
    int max_shards_req = 0;  // streamer workgroups the persistent sweep may use (0 = all CUs but the sampler's and the reducers')
    int streamer_req = 0;  // streamer variant requested: 0 automatic, 1 phase streamer, 2 row-owning waves + loader wave, 4 / 6 = 2 with
                           // two / three shards per workgroup at any N (automatic only above one resident wave of 256-row shards)
};

// what plan_sweep decided for a panel: everything the launches of its sweeps derive from
struct SweepPlan {
    int mode = 1;          // engine in force: the request, or 0 where the panel is too tall for one resident wave of streamers
    int64_t R = 0, S = 0;  // rows per shard, shards
    int V = 1;             // shards per streamer workgroup (role_streamer_rows_tall: 2, 3); the sweep's grid has S / V streamers
    int D = 1;             // Gram planes stored per block (= lag in mode 1, 1 in mode 0)
    int NG = 1;            // reducer groups = ceil(S/32)
    int near = 3;          // look-ahead lags 1..near corrected by the sampler itself, farther ones by the reducers
    int streamer = 1;      // variant in force (persistent sweep only): 1 phase streamer, 2 row-owning waves, 3 the same over byte tiles
    int nchain = 8;        // GEMV chains per shard partial: 8 (phase streamer, per-block engine) or 7 (row-owning waves)
};

constexpr size_t NGP_LDS_MAX = 160 * 1024;  // LDS of a gfx950 CU: the most one workgroup may take

// rows per shard R: a multiple of 4 -- 4*odd where that fits under the cap when the shard count is left to the library (the layouts
// of the first versions, kept so that results stay comparable; with quad-major tiles any multiple of 4 reads conflict-free), the
// smallest multiple of 4 that serves an explicit ngp_set_max_shards (there every workgroup counts: 10k rows on 209 shards are 48 rows
// each, 52 would leave 16 CUs idle); S = ceil(N/R)
void choose_layout(int64_t N, int64_t max_shards, int64_t r_cap, int64_t *R, int64_t *S, bool prefer_odd = true) {
    int64_t r0 = (N + max_shards - 1) / max_shards;
    int64_t m = (r0 + 3) / 4;
    if (m < 1) m = 1;
    if (prefer_odd && (m & 1) == 0 && 4 * (m + 1) <= r_cap) m += 1;
    int64_t r = 4 * m;
    if (r > r_cap) r = r_cap;
    *R = r;
    *S = (N + r - 1) / r;
}

// LDS of the sampler workgroup: 3 Gram planes, the dlt ring, 6 vectors of the block, 2 of ints, scalars -- and the staging area of
// the chains the kernel carries: none in the lean kernel, Tuple coefficients in the full ones (the three BayesRCpi kernels -- rc,
// tall_rc, multi_rc -- among them: their lanes' class coefficients stay in registers), BayesR coefficients on top in the _r ones
size_t sampler_lds(SweepKernel k) {
    const size_t base = (size_t)(3 * 4096 + 2 * NGP_RING * NGP_BLK + 6 * NGP_BLK) * sizeof(double) + 2 * NGP_BLK * sizeof(int) + 320;
    if (k == SweepKernel::lean || k == SweepKernel::lean_dq) return base;
    if (k == SweepKernel::r || k == SweepKernel::multi_r) return base + NGP_SAMPLER_TUPLE_LDS + NGP_SAMPLER_R_LDS;
    return base + NGP_SAMPLER_TUPLE_LDS;
}

// LDS of a streamer workgroup serving K chains (K = 1: the single-chain kernels)
size_t streamer_lds(const SweepPlan &p, int K) {
    const int R = (int)p.R;
    if (K > 1) return p.streamer == 3 ? ngp_rows_multi_lds_bytes(R, K, true) : (p.streamer == 2 ? ngp_rows_multi_lds_bytes(R, K) : ngp_multi_lds_bytes(R, K));
    if (p.streamer >= 2) {  // ring of 2 NQ + H slots | shard | 2 x 7 x 64 chain partials | 2 x 72 dlt | 2 x 8 row sums | flags | 1 KiB sink
        const size_t nq = (p.streamer == 3) ? (size_t)R / 16 : (size_t)R / 4, hq = std::min<size_t>(NGP_ROWS_HMAX, (nq + 1) / 2);
        return (2 * nq + hq) * NGP_QS + (size_t)p.V * ((R + 7) & ~7) * 8 + 2 * NGP_ROWS_NW * NGP_BLK * 8 + 2 * NGP_DLS * 8 + 16 * 8 + 64 + 1024;
    }
    // phase streamer: two tiles (quads NGP_QS bytes apart) | shard | partials | flags
    return 2 * (size_t)(R / 4) * NGP_QS + (size_t)R * 16 + 4096 + 2 * 512 + 128 + 3072 + (size_t)R * 64;
}

// dynamic LDS a launch of kernel k over K chains takes: the streamer's or the sampler's need, whichever is larger; the single-chain
// kernels add 8 KiB for the diagnostic timeline where that fits
size_t sweep_lds(const SweepPlan &p, SweepKernel k, int K = 1) {
    const size_t streamer = streamer_lds(p, K);
    size_t lds = std::max(streamer, sampler_lds(k));
    if (K == 1 && streamer + 8192 <= NGP_LDS_MAX) lds = std::max(lds, streamer + 8192);
    return lds;
}

// reducer workgroups of a fused launch serve two chains each from NGP_PAIR_FROM chains on (phase streamer only)
int fused_pair(const SweepPlan &p, int K) { return (p.streamer == 1 && K >= NGP_PAIR_FROM) ? 1 : 0; }

// workgroups of a sweep launch over K chains: per chain a sampler and a reducer per group of shards (per pair of chains where the
// reducers pair), and S / V streamers
int64_t sweep_grid(const SweepPlan &p, int K = 1) { return K + ngp_multi_reducers(K, p.NG, fused_pair(p, K)) + p.S / p.V; }

// the kernel of a sweep launch over K chains (K = 1: one chain; K >= 2: a fused pass); diag: time stamps or a timing mode are on;
// tup / rset: a chain has a Tuple / a BayesR set
SweepKernel pick_kernel(const SweepPlan &p, int K, bool diag, bool tup, bool rset, bool rcset = false) {
    // a BayesRCpi set in any chain of the launch: the kernels of the fifth translation unit, whose samplers carry eval_rcform (and the
    // Tuple and BayesR chains, so the other chains of a fused pass may hold any set) -- one chain, one chain over several shards per
    // workgroup, K chains per pass.  No time stamps or timing modes there.
    // (ngp_debug_stamps / ngp_debug_set_mode refuse the diagnostics, fusable() a fused pass over tall shards: no other kernel's
    // eval_rform may ever see a lane of method 6)
    if (rcset) {
        assert(!diag && (K == 1 || p.V == 1));
        return K > 1 ? SweepKernel::multi_rc : (p.V > 1 ? SweepKernel::tall_rc : SweepKernel::rc);
    }
    if (K > 1) {  // (BayesR: the samplers of k_sweep_r, their class coefficients staged in LDS -- where that fits beside the
                  // sampler's own; else the chain of k_sweep_multi(_tup))
        if (rset && sweep_lds(p, SweepKernel::multi_r, K) <= NGP_LDS_MAX) return SweepKernel::multi_r;
        return tup ? SweepKernel::multi_tup : SweepKernel::multi;
    }
    if (p.V > 1) return SweepKernel::tall;  // several shards per streamer workgroup: a kernel of its own (no diagnostics there)
    if (diag) return SweepKernel::diag;     // diagnostic instantiation: stamps and timing modes exist only there
    // a BayesR set: the flavour that fetches its coefficients ahead, where its LDS fits
    if (rset && sweep_lds(p, SweepKernel::r) <= NGP_LDS_MAX) return SweepKernel::r;
    // Models with a Tuple or a BayesR set run the kernel that carries those chains (k_sweep<false>, the kernel of BayesPR / BayesB /
    // BayesC, does not: ngp_sweep.h, role_sampler).  Every other model takes the lean kernel at every shape (in round 3 tall fp32
    // shards ran 1.7-2 % faster in the full kernel -- register allocation, not design; since the round-4 hand-off the lean
    // kernel is level or ahead there too: 23.4-23.6 against 23.3-23.9 ms per iteration at 50k x 600k).
    if (tup || rset) return SweepKernel::tup;
    return SweepKernel::lean;
}

// host address of a sweep kernel: each translation unit of ngp_sweep_inst.hip knows the kernels it defines
const void *sweep_kernel(SweepKernel k) {
    for (auto unit : {sweep_kernel_0, sweep_kernel_1, sweep_kernel_2, sweep_kernel_3, sweep_kernel_4, sweep_kernel_5})
        if (const void *f = unit(k)) return f;
    return nullptr;
}

// one launch of a sweep kernel; args: the SweepArgs (single-chain kernels) or the MultiArgs (fused ones) it takes
void launch_sweep_kernel(SweepKernel k, int64_t grid, size_t lds, hipStream_t stream, void *args) {
    void *a[] = {args};
    (void)hipLaunchKernel(sweep_kernel(k), dim3((unsigned)grid), dim3(NGP_WG), a, lds, stream);
}

// How a panel of N rows is swept on a device of cu_count CUs.  Pure: no allocation, no HIP call.  Returns NGP_OK, or the error code
// of a request the sweep cannot serve with its message in *msg.
int plan_sweep(int64_t N, int cu_count, const PlanRequest &q, SweepPlan *out, const char **msg) {
    SweepPlan p;
    p.mode = q.mode;
    // persistent mode: sampler + reducers + S streamers must all be resident, one workgroup per CU
    int64_t max_shards = cu_count - 1 - (cu_count + NGP_GRP - 1) / NGP_GRP;
    if (q.max_shards_req > 0) max_shards = std::min<int64_t>(max_shards, q.max_shards_req);
    if (q.storage == 1) {
        // compact storage: byte tiles, units of 16 rows, the row-owning roles only (persistent sweep)
        if (q.mode != 1) { *msg = "compact storage runs in the persistent sweep (ngp_configure mode 1) only"; return NGP_ERR_ARG; }
        const int64_t r0 = (N + max_shards - 1) / max_shards;
        p.R = 16 * std::max<int64_t>(1, (r0 + 15) / 16);
        if (p.R > NGP_U8_MAX_R) { *msg = "N too large for one resident wave of streamers in compact storage"; return NGP_ERR_ARG; }
        p.S = (N + p.R - 1) / p.R;
        p.streamer = 3;
        p.nchain = NGP_ROWS_NW;
        // delay line: 8 VGPRs per lag and update task of a lane (1, 2 or 4 tasks: ngp_u8_tasks)
        const int nt = ngp_u8_tasks((int)p.R);
        const int want = q.lag_auto ? 8 : q.lag;
        // the instantiated lags (ngp_sweep.h, variant 3): the largest one not above the request
        if (nt == 1) p.D = want >= 12 ? 12 : (want >= 8 ? 8 : (want >= 6 ? 6 : (want >= 4 ? 4 : 3)));
        else if (nt == 2) p.D = want >= 8 ? 8 : 4;
        else p.D = 4;
        p.near = q.near_req ? q.near_req : ((p.R > 128) ? 2 : 3);
    } else {
        if (p.mode == 1) {
            // Taller than one resident wave of 256-row shards: every streamer workgroup owns V = 2 (lag 3) or 3 (lag 2) shards of at
            // most 224 rows (role_streamer_rows_tall) -- S = V W shards, W workgroups, 1 + ceil(V W / 32) + W <= CUs.
            int tallV = 0;
            int64_t w_max = 0;
            for (int v = 2; v <= 3 && !tallV; v++) {
                if (q.streamer_req != 0 && q.streamer_req != 2 * v) continue;
                if (q.streamer_req == 0 && N <= max_shards * 256) continue;
                SweepPlan t;  // (W workgroups of v shards each)
                t.V = v;
                auto fits = [&](int64_t w) { t.S = v * w; t.NG = (int)((t.S + NGP_GRP - 1) / NGP_GRP); return sweep_grid(t) <= cu_count; };
                int64_t w = cu_count - 1;
                while (w > 1 && !fits(w)) w--;
                if (q.max_shards_req > 0) w = std::max<int64_t>(1, std::min<int64_t>(w, q.max_shards_req / v));
                if (N <= v * w * NGP_ROWS_MAX_R && q.lag >= 3) { tallV = v; w_max = w; }
            }
            if (tallV) {
                choose_layout(N, tallV * w_max, NGP_ROWS_MAX_R, &p.R, &p.S, q.max_shards_req <= 0);
                p.S = (p.S + tallV - 1) / tallV * tallV;  // (all-padding shards at the end if need be: zero tiles, zero rows of ycorr)
                p.V = tallV;
            } else if (N > max_shards * 256) p.mode = 0;  // too many rows for one resident wave of streamers (2 LDS tile slots + partials)
            else choose_layout(N, max_shards, 256, &p.R, &p.S, q.max_shards_req <= 0);  // 8 R / 4 update tasks <= 512 threads, two 1040 R / 4 byte LDS slots
        }
        if (p.mode == 0) choose_layout(N, 256, 508, &p.R, &p.S);  // LDS bound of k_step: R*264 + 4096 <= 160 KiB
        p.D = (p.mode == 1) ? std::min(q.lag, 8) : 1;
        // streamer variant (ngp_sweep.h): the row-owning waves serve shards of up to NGP_ROWS_MAX_R rows at lags 3..6 and are the
        // default from 64-row shards on
        // (from 64-row shards on since the publisher stopped waiting for the block's barrier: 20k x 100k 3.66 -> 3.26 ms, 28k x 100k
        // 3.97 -> 3.45, 16k x 100k 3.38 -> 3.16, equal at 52-60 rows, the phase streamer ahead at 44 rows: 1.86 against 1.99 us per block)
        if (p.mode == 1 && p.R <= NGP_ROWS_MAX_R && q.lag >= 3 && (q.streamer_req == 2 || (q.streamer_req == 0 && p.R >= 64))) p.streamer = 2;
        if (p.V > 1) p.streamer = 2;
        p.nchain = (p.streamer == 2) ? NGP_ROWS_NW : 8;
        if (p.streamer == 2) {
            if (p.D > 6) p.D = 6;  // register delay line: 32 VGPRs per lag
            if (p.V > 1) p.D = (p.V == 2) ? 3 : 2;  // ... and per shard of the workgroup
        } else if (p.mode == 1 && p.R > 128 && p.D > 5) p.D = 5;  // tall shards: the register delay line holds 5 tiles at most
        // short shards (phase streamer), lag left to the library: 6.  Lag 8 was the better one while the shard partials crossed two hops (rounds 1-3);
        // with the one-hop fixed-point sums: 10k x 100k 2.66-2.71 ms at lag 6 against 2.77-2.81 at lag 8 (7: 2.82-2.91, 5: 3.16-3.21, 4: 3.02-3.16),
        // 8k x 100k 2.64 / 2.70, 14k x 100k 2.83 / 2.87, eight chains per pass 1839 / 1775 it/s (tools/r4_run41.sh)
        else if (p.mode == 1 && q.lag_auto && p.D > 6) p.D = 6;
        // a fourth near lag overloads the sampler CU at short shards (+17 % time at 10k x 100k); the phase streamer of tall shards,
        // where with lag 5 nothing is left for the reducers then, saves 8 % with it; with the row-owning streamer (lag 6) the sampler
        // CU is again the busier end (its Gram traffic: 32 KB per near lag and block) and three near lags measure better
        // (row-owning streamer on tall shards: two near lags measured 1.5 % better still -- the far path is one hop since dlt travels as granules)
        p.near = q.near_req ? q.near_req : ((p.mode == 1 && p.streamer == 2 && p.R >= 64) ? 2 : ((p.mode == 1 && p.R > 128) ? 4 : 3));
    }
    p.NG = (int)((p.S + NGP_GRP - 1) / NGP_GRP);
    if (p.mode == 1) {
        // the sampler adds more than 8 group sums only where it fetches them one block ahead (lags 2-3: fetch_group_sums)
        if (!(p.NG <= 8 || p.D <= 3)) { *msg = "internal: more shard groups than the sampler adds"; return NGP_ERR_STATE; }
        if (sweep_lds(p, SweepKernel::tup) > NGP_LDS_MAX) { *msg = "panel too tall for the persistent sweep (LDS)"; return NGP_ERR_ARG; }
    }
    *out = p;
    return NGP_OK;
}

// Genomic variance of the kept draws (ngp_genvar.h; DESIGN.md section 2, "Genomic variance"): the caller's windows per marker set, the
// segments / items / slots built from them for the sets the chain has now, and the chain's partials, sums and trace on the device
struct GenVar {
    bool on = false;
    double thr = 0.01;
    int64_t trace_rows = 0;
    std::vector<std::vector<int64_t>> win;  // per marker set: start, stop of every window, relative to the set's first column
    bool built = false;
    std::vector<int64_t> built_for;         // col0, ncol of every set the tables below were built for
    std::vector<GvSeg> segs;
    std::vector<GvItem> items;
    int64_t nwin = 0, nslots = 0, ncol_w = 0, nblk_r = 0;
    int ex = 0;                             // 2^ex > max |x_ij| over the live rows of the panel (k_genvar_xmax, when the tables are built)
    DevArray<GvSeg> d_segs;
    DevArray<GvItem> d_items;
    DevArray<int> d_set_item0, d_set_seg0, d_slot_seg, d_slot_e;
    DevArray<double> d_part, d_segm, d_sega, d_acc, d_trace;  // d_acc: [6][nslots] | sum r | sum r^2
    DevArray<long long> d_qw, d_qs, d_cnt;
    int64_t launches = 0, served = 0;       // ngp_get_genomic_variance_stats
};

// Convergence diagnostics of the kept draws (ngp_diag.h; DESIGN.md section 2, "Convergence diagnostics"): the window, the draws taken,
// the gather table of the monitored vector (ngp_state.h, diag_layout) and the chain's streaming state on the device
struct Diag {
    bool on = false;
    int L = 64;                    // lags 0 .. L-1
    int64_t split = 0, n = 0;      // draws with index < split feed half 0; draws taken (host bookkeeping, rewound with h->iter)
    int64_t D = 0, Dp = 0;         // monitored scalars; the row stride on the device (D rounded up to even); 0: nothing allocated
    bool fixed = false;            // a draw was taken or a state was set: D may no longer change
    std::vector<DiagSeg> segs;     // the table d_segs holds
    int64_t maxw = 0;              // words of its longest run
    DevArray<DiagSeg> d_segs;
    size_t seg_cap = 0;            // entries d_segs was allocated for
    DevArray<double> d_x, d_st;   // theta of the draw [Dp] (pad 0); x1 | S1[2] | S2[2] | C[L] | head[L] | ring[L], rows of Dp
    int64_t launches = 0;          // ngp_get_diagnostics_stats
};

// Liability traits (ngp_liability.h; ngp_set_liability_classes / ngp_set_liability_bounds): the augmented rows with their classes
// (C >= 2) or bounds (C == 0) on the host and on the device, the liability of each, and d_thr = thr[C+1] | sum_thr[C+1] |
// sum_thr2[C+1] (thr[0] = -inf, thr[1] = 0, thr[C] = +inf; the sums are used at 2 .. C-1); all empty for a chain without them
struct Liab {
    std::vector<long long> rows;
    std::vector<int> cls;
    std::vector<double> lo, hi;
    int C = 0;
    uint64_t digest = 0;  // of rows, C and classes or bounds (snapshot signature)
    DevArray<long long> d_rows;
    DevArray<int> d_cls;
    DevArray<double> d_lo, d_hi, d_liab, d_thr;
    // Cowles' threshold step (ngp_threshold.h; ngp_set_threshold_step): 0 = Albert-Chib, 1 = Cowles; adapt: sigma was given as 0 and
    // follows the acceptance rate through burn-in; d_ts the step's words, d_tg = g[C+1] | in-order flag, d_tpart the workgroups' partials
    int ts_mode = 0;
    bool ts_adapt = false;
    double ts_sigma0 = 0.0;  // the SD a fresh chain starts with (ngp_set_y): the caller's, or 1 / sqrt(m) under adaptation
    DevArray<ThrStep> d_ts;
    DevArray<double> d_tg, d_tpart;
    // class probabilities of the held-out records (ngp_enable_class_probabilities): sum_prob[C][m_holdout], class-major; null when off
    DevArray<double> d_sum_prob;
    bool on() const { return !rows.empty(); }
    size_t thr_bytes() const { return C >= 2 ? (size_t)(C - 1) * 8 : 0; }  // t_1 .. t_{C-1}, as the formats carry them
};

// The chain's arrays on one panel (sized by its N, P and plan): allocated whole by alloc_panel, dropped whole with the panel
struct ChainMem {
    GenVar gv;
    Diag dg;
    Liab lb;
    DevArray<double> d_lhs0, d_rhs0, d_beta, d_c, d_w, d_q, d_T, d_chi;
    DevArray<int8_t> d_setof;
    DevArray<int32_t> d_loc, d_vbidx;
    DevArray<uint8_t> d_delta;
    DevArray<double> d_sum_beta, d_sum_beta2, d_sum_delta;
    DevArray<double> d_ycorr, d_part, d_dlt;
    DevArray<double> d_rs;  // weighted residuals: row scales s = sqrt(w) (L entries, padding rows 0); null for an unweighted handle
    DevArray<DSet> d_sets;
    DevArray<DScal> d_scal;
    // persistent sweep: the dlt ring, dlt as tagged granules, and the hand-off words -- fixed-point accumulators (RING x 8 copies x
    // 64 x 8 bytes) | dlt flag (one line) | census counters (one line) | census table (placement of each workgroup, 2 words each),
    // all zeroed by k_prep
    DevArray<double> d_cdlt;
    DevArray<unsigned long long> d_cdltg;
    DevArray<unsigned> d_ccnt;
    size_t ccnt_words = 0;
    size_t census_off = 0;  // word offset of the census counters inside d_ccnt
    unsigned long long *d_census_tbl = nullptr;  // view: the census table inside d_ccnt (placement of the last launch's workgroups)
    DevArray<unsigned> abort_mem;  // this chain's abort word (32 words)
    unsigned *d_abort = nullptr;   // view: the abort word the launches read -- abort_mem, or a fused run's leader's (run_fused)
    // inverse form of the linear blocks' chain (k_tinv): T per block, written before every sweep
    DevArray<double> d_tinv;
    int64_t tinv_blocks = 0;       // blocks d_tinv was allocated for
    DevArray<unsigned> d_blin;     // [NBLK] 1 = linear block (static for a model and an active set: written by sync_linear_blocks)
    int blin_for = -2;             // active set d_blin was written for (-1: the whole model, -2: stale)
    int lin_all = 0, lin_any = 0;  // every / any block of d_blin is linear
    // prediction (ngp_predict.h): this chain's sums over kept draws [nsets + 1][Np] (last row: the total), g of the last kept draw, the
    // chunk partials of a launch and the work items of this chain's marker sets; sized by ensure_prediction for (panel, number of sets)
    DevArray<double> d_pred_sum, d_pred_sum2, d_pred_last, d_pred_part, d_pred_mpart;
    DevArray<PredItem> d_pred_items;
    DevArray<int> d_pred_set0;
    std::vector<PredItem> pred_items;
    uint64_t pred_for = 0;  // the panel (its id) and the number of sets the arrays above were sized for
    int64_t pred_rows = 0;
    int64_t pred_launches = 0, pred_served = 0;  // ngp_get_prediction_stats: launches this handle made, chains they served
    // held-out records (ngp_holdout.h; ngp_set_holdout): the rows on the host and on the device, the augmented phenotype of each, and
    // the sums of their fitted values over kept draws [N] (zero off the rows); all empty for a chain without a mask
    std::vector<long long> ho_rows;
    DevArray<long long> d_ho_rows;
    DevArray<double> d_yaug, d_sum_fit, d_sum_fit2, d_n_fit;
};

// The model's arrays beyond the chain's: what a new panel discards (alloc_panel resets the whole group)
struct ModelMem {
    DevArray<double> d_varBeta, d_sum_varBeta;
    int64_t vb_cap = 0;                // entries d_varBeta / d_sum_varBeta were allocated for
    DevArray<double> d_rcls;           // BayesR per-locus class coefficients [4][NGP_RMAX][Ppad] (allocated with the first BayesR set)
    // PR region tables
    DevArray<DReg> d_regs;
    DevArray<long long> d_seg_k0;
    DevArray<int32_t> d_seg_len;
    DevArray<int32_t> d_seg_set;       // set of every variance segment
    DevArray<double> d_segpart, d_regchi;
    // Tuple sets (src/functions.jl:140-154): per-set constants, coefficient rows, region tables of the inverse-Wishart draws
    DevArray<DTup> d_tup;
    DevArray<double> d_tupc, d_tupg, d_tsegpart;
    DevArray<DTReg> d_tregs;
    DevArray<long long> d_tseg_l0;
    DevArray<int32_t> d_tseg_len, d_tseg_set;
    std::vector<HFix> fix;             // fixed-effect sets beyond the intercept (src/functions.jl:22-53), in sampling order
    int64_t nfixcol = 0;               // sum of ncol over them: entries of d_bfix / d_sum_bfix
    DevArray<double> d_bfix, d_sum_bfix;
    std::vector<HRand> rnd;            // (1|g) random-effect sets (src/functions.jl:57-110), sampled after the fixed-effect sets, in order
    std::vector<HLv> lv;               // variance models of the BayesLV sets (src/functions.jl:442-485), in the order of their sets
    std::vector<HRc> rc;               // per-locus annotation state of the BayesRCpi sets (src/functions.jl:291-360), in the order of their sets
    DevArray<DRc> d_rctab;             // [16] their device arrays by marker set (k_prep); allocated with the first such set
    // optional per-iteration traces of selected effects, variances and pi (ngp_set_trace_loci)
    DevArray<int64_t> d_trace_loci;
    int64_t ntl = 0, ntvb = 0;
    DevArray<double> d_tr_beta, d_tr_vb, d_tr_pi;
    int64_t trace_ext_cap = 0;         // iterations d_tr_beta / d_tr_vb / d_tr_pi were allocated for
};

// Buffers that live as long as the handle
struct HandleMem {
    DevArray<double> d_tr_varE, d_tr_b;  // varE / b traces of the last run
    int64_t trace_cap = 0;               // iterations they were allocated for
    DevArray<unsigned long long> d_dbg;  // time stamps (ngp_debug_stamps)
    DevArray<unsigned long long> d_tn_fall;  // truncated-normal draws whose loop ran out (ngp_get_liability_stats); allocated on first use
};

}  // namespace

struct ngp_handle {
    int device = 0;
    uint64_t seed = 0;
    uint32_t chain = 0;
    hipStream_t stream = nullptr;
    int64_t N = 0, P = 0, NBLK = 0, Ppad = 0, L = 0;
    size_t lds_step = 0;
    PlanRequest req;  // how the caller wants the panel swept (its mode becomes 0 where plan_sweep falls back to mode 0)
    SweepPlan plan;   // how it is swept: plan_sweep's decision, or the owner's plan for a shared panel
    // device memory, by lifetime: the panel (null: no panel set), the chain's arrays on it, the model's, the handle's own
    std::shared_ptr<PanelMem> pm;
    ChainMem cm;
    ModelMem mm;
    HandleMem hm;
    bool records_only = false;  // ngp_set_records: N records and no genotype panel (one inert block of 64 zero columns stands in for it)
    Grm grm;                    // ngp_grm_*: independent of the panel and of the model
    bool panel_open = false;  // between ngp_begin_panel and ngp_end_panel: columns may still arrive, the Gram window does not exist yet
    bool pred_open = false;   // between ngp_begin_prediction_panel and ngp_end_prediction_panel: only prediction columns may be called
    int cu_count = 256;
    double setup_ms[3] = {0.0, 0.0, 0.0};   // wall time of the last panel set-up: device allocation (+ zeroing) | tiles (generation / upload) | Gram window
    unsigned launch_seq = 0;                // launch nonce of the granule tags
    int chain_form = 0;       // ngp_set_chain_form: 0 = every block by the 64-step chain (default), 1 = linear blocks as dlt = T e0
    std::vector<int32_t> h_seg_set;
    int64_t nclass_total = 0;        // sum of K over the BayesR sets (entries of the packed posterior)
    std::vector<DTReg> h_tregs;
    std::vector<long long> h_tseg_l0;
    std::vector<int32_t> h_tseg_len, h_tseg_set;
    int ntuple = 0;
    std::vector<DReg> h_regs;
    std::vector<long long> h_seg_k0;
    std::vector<int32_t> h_seg_len;
    bool tables_dirty = false;
    // model (host mirror)
    std::vector<HSet> sets;
    std::vector<int8_t> h_setof;
    std::vector<int32_t> h_loc, h_vbidx;
    int64_t nvb = 0;
    double e_df = 4.0, e_scale = 0.0005;
    double fix_varE = 0.0;  // ngp_fix_residual_variance: > 0 holds varE at this value (k_head draws none), 0 samples it
    // weighted residuals (ngp_set_residual_weights, E.str == "D"): w as given (empty = unweighted) and their sum (index order); the
    // row scales on the device are cm.d_rs
    std::vector<double> h_rw;
    double sum_w = 0.0;
    int intercept = 1;
    int64_t chainLength = 0, burnIn = 0, thin = 1;
    int64_t iter = 0;
    bool have_y = false;
    int64_t ntrace = 0;  // iterations in hm.d_tr_varE / hm.d_tr_b
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double iter_ms = 0.0;
    int64_t iters_timed = 0;
    int64_t sweep_launches = 0;
    // diagnostics (ngp_debug_set_mode): != 0 makes every chain invalid, ngp_run / ngp_sweep_set then return NGP_ERR_DEBUG
    int dbg_mode = 0;
    int gram_engine = 0;  // 0: Gram window by the fp64 VALU kernel (k_gram_part), 1: on the matrix cores (k_gram_part_mfma, bit-identical); the knob's bit 10
    int knob = 0;  // ngp_debug_set_knob, timing only: bits 0-2 pace the loader wave of the row-owning streamer (s_sleep units after every four
                   // requests), bit 4 counts every partial before the block's barrier, bit 8 flips the publisher's early signal (the
                   // streamers read these through SweepArgs.knob); bit 10 builds the Gram window on the matrix cores (gram_engine)
                   // bit 11 switches the streamers' L2 warming off, bit 13 withholds the warmer role, bit 14 offers it below 160-row shards, bits 16-27 select the shard of the diagnostic timeline (ngp_sweep.h)
    bool poisoned = false;  // a sweep gave up half-way (abort word): the chain state is unusable until ngp_set_y / ngp_set_state
    bool exclusive = false;  // a grid of this handle was once not co-resident beside other chains' grids: its calls now lease the whole device
    int64_t last_grid = 0;       // workgroups of the last sweep launch this handle led (fused launches: K (1 + NG) + S)
    int64_t census_retries = 0;  // launches that ended at the census and were run again with the device to themselves
    int64_t dbg_census_fail_iter = 0;  // ngp_debug_fail_census: the sweep of this iteration ends at its census (once)
    std::unique_ptr<SampleStream> smp;  // ngp_set_sample_file
    int vdev = -1;           // ngp_debug_set_virtual_device: the device ngp_allreduce_posterior groups this handle under (-1: the real one)
    int64_t dbg_staging_bytes = 0;  // ngp_debug_set_staging_bytes: in place of the 256 MiB / 64 MiB of every staged loader (0: those)
    std::string err;
};

namespace {

int fail(ngp_handle *h, int code, const std::string &msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}
// the same for the exception barrier of the C ABI: storing the message must not throw a second time
int fail_nothrow(ngp_handle *h, int code, const char *what) noexcept {
    try {
        std::string &dst = h ? h->err : g_create_err;
        dst.assign(what ? what : "?");
    } catch (...) {  // out of memory while storing the message: keep the code, drop the text
        try { (h ? h->err : g_create_err).clear(); } catch (...) {}
    }
    return code;
}

// Exception barrier (include/nextgp_hip.h: "no C++ exception crosses this boundary"; SURVEY.md section 8b, error conventions):
// every extern "C" body runs inside NGP_TRY ... NGP_CATCH(handle).  std::vector / std::string / std::thread can throw
// (bad_alloc, length_error, system_error); unwinding into the caller's ccall frame would abort the Julia process, so they become
// a negative status and a message for ngp_last_error, like every other failure (the reference's error(...) style, src/mme.jl:77,343).
#define NGP_TRY try {
#define NGP_CATCH(H)                                                                                                 \
    }                                                                                                                \
    catch (const std::bad_alloc &) { return fail_nothrow((H), NGP_ERR_NOMEM, "out of host memory (std::bad_alloc)"); } \
    catch (const std::exception &e_) {                                                                               \
        char b_[256];                                                                                                \
        std::snprintf(b_, sizeof b_, "internal error (C++ exception stopped at the C ABI): %s", e_.what());          \
        return fail_nothrow((H), NGP_ERR_HIP, b_);                                                                   \
    }                                                                                                                \
    catch (...) { return fail_nothrow((H), NGP_ERR_HIP, "internal error (unknown C++ exception stopped at the C ABI)"); }

#define HCHK(call)                                                                                          \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(h, NGP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));                 \
    } while (0)

#define REQUIRE(cond, code, msg)                \
    do {                                        \
        if (!(cond)) return fail(h, code, msg); \
    } while (0)

// Persistent sweeps of SEVERAL handles of this process on one device (chains in their own host threads, ngp_set_max_shards):
// every workgroup of a sweep waits for others of its grid, so two sweeps may only run together if both grids fit the device at
// once.  A call that launches sweeps leases its grid's CUs for its duration; a lease that does not fit waits for the running
// calls to return (the chains then take turns instead of giving up on their spins).  Other processes cannot be seen from here:
// against them the bounded spins and the abort word remain.
struct CuLease {
    static std::mutex &mu() { static std::mutex m; return m; }
    static std::condition_variable &cv() { static std::condition_variable c; return c; }
    static int *in_use() { static int u[64] = {0}; return u; }
    int dev = -1, n = 0, cap = 0, want = 0;
    bool excl = false;
    explicit CuLease(ngp_handle *h, int64_t grid_override = 0) {
        if (h->plan.mode != 1) return;
        // workgroups are handed to the 8 XCDs in turn, so a grid occupies ceil(grid / 8) CUs of EVERY XCD: the unit of the lease
        // (three grids of 85 workgroups -- 255 of 256 CUs -- do not fit: 3 x 11 > 32 per XCD; measured, they wait for each other)
        dev = h->device & 63; want = (int)(((grid_override > 0 ? grid_override : sweep_grid(h->plan)) + 7) / 8);
        cap = std::max(1, h->cu_count / 8);
        acquire(h->exclusive);
    }
    void acquire(bool exclusive) {
        if (dev < 0) return;
        excl = exclusive; n = exclusive ? cap : want;  // exclusive: the whole device, i.e. nobody else's sweep beside this call's
        std::unique_lock<std::mutex> lk(mu());
        cv().wait(lk, [&] { return in_use()[dev] == 0 || in_use()[dev] + n <= cap; });
        in_use()[dev] += n;
    }
    void release() {
        if (dev < 0 || n == 0) return;
        { std::lock_guard<std::mutex> lk(mu()); in_use()[dev] -= n; }
        n = 0;
        cv().notify_all();
    }
    // the count fitted and the grids still were not all resident (census): give the share back and wait for the device to be free
    void make_exclusive() { release(); acquire(true); }
    ~CuLease() { release(); }
};

// bytes one staging chunk of a host loader may hold: the loader's own constant unless a test shrank it (ngp_debug_set_staging_bytes)
int64_t staging_bytes(const ngp_handle *h, int64_t dflt) { return h->dbg_staging_bytes > 0 ? h->dbg_staging_bytes : dflt; }

int enter(ngp_handle *h, bool pred_call = false) {
    if (!h) return fail(nullptr, NGP_ERR_ARG, "null handle");
    if (h->pred_open && !pred_call)
        return fail(h, NGP_ERR_STATE, "a prediction panel is open: only ngp_prediction_columns_* and ngp_end_prediction_panel may be called until it is ended");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return NGP_OK;
}

template <typename T>
int DevArray<T>::alloc(ngp_handle *h, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = alloc_raw(std::max<size_t>(n, 1));
    if (e != hipSuccess) return fail(h, NGP_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    e = hipMemsetAsync(p, 0, bytes, h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    return NGP_OK;
}

// No panel, hence no chain arrays and no model: where a panel set-up starts (a new panel is a new model -- the fixed-effect and
// random-effect sets hold rows of the old N, the trace selection loci of the old P) and what a failed one leaves behind
void drop_panel(ngp_handle *h) {
    h->pm.reset();  // (handles that share the old panel keep it alive)
    if (h->cm.lb.C > 0) h->fix_varE = 0.0;  // (the classes that fixed varE at 1 go with the panel)
    h->cm = ChainMem();
    h->mm = ModelMem();
    h->sets.clear(); h->nvb = 0; h->nclass_total = 0; h->ntuple = 0;
    h->h_setof.clear(); h->h_loc.clear(); h->h_vbidx.clear();
    h->h_regs.clear(); h->h_seg_k0.clear(); h->h_seg_len.clear(); h->h_seg_set.clear();
    h->h_tregs.clear(); h->h_tseg_l0.clear(); h->h_tseg_len.clear(); h->h_tseg_set.clear();
    h->have_y = false; h->iter = 0; h->poisoned = false; h->panel_open = false; h->records_only = false; h->pred_open = false;
}

// A new panel of N x P (owner: ngp_share_panel's, whose arrays and plan are taken as they are).  The old panel goes first, so that
// two never coexist on the device; the new one is built aside and installed only once complete -- a set-up that fails leaves the
// handle without a panel.
int alloc_panel(ngp_handle *h, int64_t N, int64_t P, ngp_handle *owner = nullptr) {
    REQUIRE(N > 0 && P > 0, NGP_ERR_ARG, "panel dimensions must be positive");
    REQUIRE(N <= (int64_t)508 * 1024, NGP_ERR_ARG, "N too large for this build (max 520192)");
    if (owner) {  // the owner's rows were scaled by the owner's weights: a sharer takes them (and may not bring others)
        REQUIRE(h->h_rw.empty() || h->h_rw == owner->h_rw, NGP_ERR_ARG, "ngp_share_panel: this handle's residual weights differ from the owner's");
        h->h_rw = owner->h_rw; h->sum_w = owner->sum_w;
    }
    if (!h->h_rw.empty()) {
        REQUIRE((int64_t)h->h_rw.size() == N, NGP_ERR_ARG, "residual weights hold " + std::to_string(h->h_rw.size()) + " entries, the panel " +
                                                               std::to_string(N) + " rows");
        REQUIRE(h->req.storage == 0, NGP_ERR_ARG, "residual weights with compact storage (NGP_STORAGE_U8) are not supported: use fp32 tiles");
    }
    drop_panel(h);
    PlanRequest req = h->req;
    SweepPlan plan;
    if (owner) {  // the owner's requests and plan, as they are
        req = owner->req;
        plan = owner->plan;
    } else {
        const char *msg = nullptr;
        if (int e = plan_sweep(N, h->cu_count, req, &plan, &msg)) return fail(h, e, msg);
        req.mode = plan.mode;  // (a panel too tall for the persistent sweep leaves the handle in mode 0)
    }
    const int64_t NBLK = (P + NGP_BLK - 1) / NGP_BLK, L = plan.R * plan.S;
    const size_t pp = (size_t)(NBLK * NGP_BLK), lds_step = (size_t)plan.R * 264 + 4096;
    int rc;
    std::shared_ptr<PanelMem> pm = owner ? owner->pm : std::make_shared<PanelMem>();
    if (!owner) {
        const size_t tile_elems = (size_t)plan.R * NGP_BLK;
        // column means: what the analytic centring of the compact storage uses; kept for the fp32 tiles too (ngp_get_storage: a host
        // can then rebuild any centred row of the panel from the genotype codes)
        if ((rc = pm->mean.alloc(h, pp))) return rc;
        if (req.storage == 1) {  // one byte per element (R is a multiple of 16), held behind the same pointer
            if ((rc = pm->tiles.alloc(h, (size_t)NBLK * plan.S * tile_elems / 4))) return rc;
        } else if ((rc = pm->tiles.alloc(h, (size_t)NBLK * plan.S * tile_elems))) return rc;
        if ((rc = pm->gramx.alloc(h, (size_t)NBLK * plan.D * NGP_BLK * NGP_BLK))) return rc;
        if ((rc = pm->mpm.alloc(h, pp))) return rc;
    }
    ChainMem c;
    for (DevArray<double> *a : {&c.d_lhs0, &c.d_rhs0, &c.d_beta, &c.d_c, &c.d_w, &c.d_q, &c.d_T, &c.d_chi})
        if ((rc = a->alloc(h, pp))) return rc;
    if ((rc = c.d_setof.alloc(h, pp))) return rc;
    if ((rc = c.d_loc.alloc(h, pp))) return rc;
    if ((rc = c.d_vbidx.alloc(h, pp))) return rc;
    if ((rc = c.d_delta.alloc(h, pp))) return rc;
    for (DevArray<double> *a : {&c.d_sum_beta, &c.d_sum_beta2, &c.d_sum_delta})
        if ((rc = a->alloc(h, pp))) return rc;
    if ((rc = c.d_ycorr.alloc(h, (size_t)L))) return rc;
    if (!h->h_rw.empty()) {  // row scales s_i = sqrt(w_i), before any tile is filled (the fills read them)
        std::vector<double> rs((size_t)L, 0.0);
        for (int64_t i = 0; i < N; i++) rs[(size_t)i] = std::sqrt(h->h_rw[(size_t)i]);
        if ((rc = c.d_rs.alloc(h, (size_t)L))) return rc;
        HCHK(hipMemcpy(c.d_rs, rs.data(), rs.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = c.d_part.alloc(h, (size_t)plan.S * NGP_BLK))) return rc;
    if ((rc = c.d_dlt.alloc(h, NGP_BLK))) return rc;
    if ((rc = c.d_sets.alloc(h, 16))) return rc;
    if ((rc = c.d_scal.alloc(h, 1))) return rc;
    HCHK(hipMemsetAsync(c.d_setof, 0xFF, pp, h->stream));
    HCHK(hipMemsetAsync(c.d_delta, 1, pp, h->stream));
    if (req.storage == 0) HCHK(hipFuncSetAttribute((const void *)k_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_step));
    if (plan.mode == 1) {
        // the single-chain kernels, each with the LDS this plan launches it with (k_sweep_r where that fits)
        for (SweepKernel k : {SweepKernel::lean, SweepKernel::lean_dq, SweepKernel::diag, SweepKernel::tup, SweepKernel::r, SweepKernel::rc, SweepKernel::tall, SweepKernel::tall_rc}) {
            const size_t lds = sweep_lds(plan, k);
            if (lds <= NGP_LDS_MAX) HCHK(hipFuncSetAttribute(sweep_kernel(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        // every workgroup of the persistent kernel waits for others: the whole grid must be resident at once, one workgroup
        // per CU.  Checked here, not assumed (a grid that does not fit would only show up as a spin timeout).
        int wg_per_cu = 0;
        const SweepKernel occ = plan.V > 1 ? SweepKernel::tall : SweepKernel::lean;  // (at the LDS of the full kernel: the most but k_sweep_r's)
        HCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg_per_cu, sweep_kernel(occ), NGP_WG, sweep_lds(plan, SweepKernel::tup)));
        const int64_t grid = sweep_grid(plan);
        if (wg_per_cu < 1 || grid > (int64_t)wg_per_cu * h->cu_count)
            return fail(h, NGP_ERR_STATE, "persistent sweep: grid of " + std::to_string(grid) + " workgroups cannot be co-resident (" +
                                              std::to_string(wg_per_cu) + " per CU x " + std::to_string(h->cu_count) + " CUs); use ngp_configure(mode 0)");
        if ((rc = c.d_cdlt.alloc(h, (size_t)NGP_RING * NGP_BLK))) return rc;
        if ((rc = c.d_cdltg.alloc(h, (size_t)NGP_RING * NGP_BLK * 2))) return rc;
        c.census_off = (size_t)NGP_RING * NGP_FX_COPIES * NGP_BLK * 2 + 32;
        c.ccnt_words = c.census_off + 32 + 2 * (size_t)320;  // (320 >= any grid, also the fused grid of K chains per pass)
        if ((rc = c.d_ccnt.alloc(h, c.ccnt_words))) return rc;
        c.d_census_tbl = (unsigned long long *)(c.d_ccnt.get() + c.census_off + 32);
    }
    if ((rc = c.abort_mem.alloc(h, 32))) return rc;
    c.d_abort = c.abort_mem;
    HCHK(hipStreamSynchronize(h->stream));
    // complete: install it
    h->N = N; h->P = P; h->NBLK = NBLK; h->Ppad = (int64_t)pp; h->L = L; h->lds_step = lds_step;
    h->req = req; h->plan = plan;
    h->pm = std::move(pm);
    h->cm = std::move(c);
    h->h_setof.assign(pp, -1);
    h->h_loc.assign(pp, 0);
    h->h_vbidx.assign(pp, 0);
    return NGP_OK;
}

// max_j x_j'x_j: with ycorr'ycorr it bounds every X_t'ycorr (the scale of the fixed-point accumulators, k_head)
int refresh_mpm_max(ngp_handle *h) {
    std::vector<double> m((size_t)h->Ppad);
    HCHK(hipMemcpy(m.data(), h->pm->mpm, (size_t)h->Ppad * sizeof(double), hipMemcpyDeviceToHost));
    double mx = 0.0;
    for (double v : m) if (v > mx) mx = v;
    h->pm->mpm_max = mx;
    return NGP_OK;
}

// weighted residuals: N rows of a device vector into the row-scaled problem (dst = s src) or back out of it (dst = src / s), on the
// handle's stream; dst may be src.  Unweighted handles never get here.
void launch_rows(ngp_handle *h, double *dst, const double *src, bool descale) {
    const unsigned nb = (unsigned)((h->N + 255) / 256);
    if (descale) hipLaunchKernelGGL(k_row_descale, dim3(nb), dim3(256), 0, h->stream, dst, src, (const double *)h->cm.d_rs, (long long)h->N);
    else hipLaunchKernelGGL(k_row_scale, dim3(nb), dim3(256), 0, h->stream, dst, src, (const double *)h->cm.d_rs, (long long)h->N);
}

// FNV-1a over the bytes of the weights: what a snapshot of a weighted chain records of them (ngp_save_snapshot)
uint64_t weights_digest(const std::vector<double> &w) {
    uint64_t x = 1469598103934665603ull;
    const unsigned char *p = (const unsigned char *)w.data();
    for (size_t k = 0; k < w.size() * sizeof(double); k++) { x ^= p[k]; x *= 1099511628211ull; }
    return x;
}
// the same over the held-out rows (int64 each): what a snapshot of a chain with a mask records of it
uint64_t rows_digest(const std::vector<long long> &rows) {
    uint64_t x = 1469598103934665603ull;
    const unsigned char *p = (const unsigned char *)rows.data();
    for (size_t k = 0; k < rows.size() * sizeof(long long); k++) { x ^= p[k]; x *= 1099511628211ull; }
    return x;
}

int build_gram8(ngp_handle *h) {  // compact storage: exact integer dot products, then G = dot - N (m_k m_j)
    const size_t per_block = (size_t)h->plan.S * NGP_BLK * NGP_BLK * sizeof(uint32_t);
    int nb_max = (int)std::max<size_t>(1, std::min<size_t>((size_t)h->NBLK, ((size_t)1 << 30) / per_block));
    nb_max = std::min(nb_max, 32768);
    DevArray<uint32_t> d_gpart;
    int rc;
    if ((rc = d_gpart.alloc(h, (size_t)nb_max * h->plan.S * NGP_BLK * NGP_BLK))) return rc;
    for (int d = 0; d < h->plan.D; d++)
        for (int64_t t0 = 0; t0 < h->NBLK; t0 += nb_max) {
            int nb = (int)std::min<int64_t>(nb_max, h->NBLK - t0);
            hipLaunchKernelGGL(k_gram8_part, dim3((unsigned)h->plan.S, (unsigned)nb), dim3(256), 0, h->stream, (const uint8_t *)h->pm->tiles.get(), d_gpart,
                               (int)h->plan.R, (int)h->plan.S, (int)t0, d);
            long long ne = (long long)nb * NGP_BLK * NGP_BLK;
            hipLaunchKernelGGL(k_gram8_reduce, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, h->stream, d_gpart, h->pm->gramx, h->pm->mpm,
                               h->pm->mean, (long long)h->N, (int)h->plan.S, (int)t0, nb, d, h->plan.D);
        }
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("gram: ") + hipGetErrorString(e));
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("gram launch: ") + hipGetErrorString(e));
    return refresh_mpm_max(h);
}

int build_gram(ngp_handle *h) {
    if (h->req.storage == 1) return build_gram8(h);
    // batches of blocks so the shard-partial scratch stays <= ~1 GiB
    const size_t per_block = (size_t)h->plan.S * NGP_BLK * NGP_BLK * sizeof(double);
    int nb_max = (int)std::max<size_t>(1, std::min<size_t>((size_t)h->NBLK, ((size_t)1 << 30) / per_block));
    nb_max = std::min(nb_max, 32768);
    DevArray<double> d_gpart;
    int rc;
    if ((rc = d_gpart.alloc(h, (size_t)nb_max * h->plan.S * NGP_BLK * NGP_BLK))) return rc;
    for (int d = 0; d < h->plan.D; d++)
        for (int64_t t0 = 0; t0 < h->NBLK; t0 += nb_max) {
            int nb = (int)std::min<int64_t>(nb_max, h->NBLK - t0);
            if (h->gram_engine == 0)  // fp64 VALU contraction: the default (1.63 ms per launch at 50k x 600k against 1.84 on the matrix cores)
                hipLaunchKernelGGL(k_gram_part, dim3((unsigned)h->plan.S, (unsigned)nb), dim3(256), 0, h->stream, h->pm->tiles, d_gpart, (int)h->plan.R,
                                   (int)h->plan.S, (int)t0, d);
            else                      // matrix cores (ngp_debug_set_knob bit 10 before the panel is set): v_mfma_f64_16x16x4_f64, the same sums in the same order
                hipLaunchKernelGGL(k_gram_part_mfma, dim3((unsigned)h->plan.S, (unsigned)nb), dim3(256), 0, h->stream, h->pm->tiles, d_gpart, (int)h->plan.R,
                                   (int)h->plan.S, (int)t0, d);
            long long ne = (long long)nb * NGP_BLK * NGP_BLK;
            hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, h->stream, d_gpart, h->pm->gramx, h->pm->mpm,
                               (int)h->plan.S, (int)t0, nb, d, h->plan.D);
        }
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("gram: ") + hipGetErrorString(e));
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("gram launch: ") + hipGetErrorString(e));
    return refresh_mpm_max(h);
}

// ---- host panels in Float64 / Float32, whole or in column ranges (ngp_begin_panel / ngp_panel_columns_* / ngp_end_panel) ----
int begin_panel(ngp_handle *h, int64_t N, int64_t P) {
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = alloc_panel(h, N, P))) return rc;  // (tiles and means are born zero: columns never uploaded stay zero columns)
    h->panel_open = true;
    return NGP_OK;
}

// columns [col0, col0 + ncol) from a column-major host matrix: staged through the device in chunks of whole columns (256 MiB)
template <typename TIn>
int panel_columns(ngp_handle *h, int64_t col0, const TIn *M, int64_t ncol, int64_t ld, int centre) {
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->panel_open && h->pm, NGP_ERR_STATE, "ngp_panel_columns_* needs an open panel (ngp_begin_panel)");
    REQUIRE(M != nullptr, NGP_ERR_ARG, "null panel pointer");
    REQUIRE(ld >= h->N, NGP_ERR_ARG, "leading dimension smaller than N");
    REQUIRE(col0 >= 0 && ncol > 0 && col0 + ncol <= h->P, NGP_ERR_ARG, "column range outside the panel");
    REQUIRE(h->req.storage == 0 || sizeof(TIn) == 1, NGP_ERR_ARG,
            "compact storage takes genotype codes: ngp_panel_columns_u8, ngp_set_panel_u8, ngp_load_panel_file or ngp_generate_panel");
    const int64_t N = h->N;
    const int64_t cchunk = std::max<int64_t>(1, std::min<int64_t>(ncol, staging_bytes(h, (int64_t)256 << 20) / (int64_t)(ld * sizeof(TIn))));
    DevArray<TIn> d_g;
    DevArray<unsigned> d_bad;
    if (d_g.alloc_raw((size_t)cchunk * ld) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "staging buffer");
    if ((rc = d_bad.alloc(h, 1))) return rc;
    hipError_t e = hipSuccess;
    for (int64_t c0 = 0; c0 < ncol && e == hipSuccess; c0 += cchunk) {
        const int64_t nc = std::min<int64_t>(cchunk, ncol - c0);
        // the last column may be shorter than ld in the caller's buffer: nc - 1 full columns + N elements
        e = hipMemcpyAsync(d_g, M + (size_t)c0 * ld, ((size_t)(nc - 1) * ld + (size_t)N) * sizeof(TIn), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) break;
        double *d_mu = h->pm->mean + col0 + c0;
        hipLaunchKernelGGL(k_cols_mean<TIn>, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, h->stream, (const TIn *)d_g, (long long)N, (long long)ld,
                           (long long)nc, centre, d_mu, d_bad);
        if constexpr (sizeof(TIn) == 1) {
            if (h->req.storage == 1)  // the codes stay codes (the means are what the analytic centring uses)
                hipLaunchKernelGGL(k_cols_fill8, dim3((unsigned)((h->L / 16 + 255) / 256), (unsigned)nc), dim3(256), 0, h->stream, (uint8_t *)h->pm->tiles.get(),
                                   (const uint8_t *)d_g, (long long)N, (long long)ld, (long long)(col0 + c0), (int)h->plan.R, (int)h->plan.S);
        }
        if (h->req.storage == 0)
        hipLaunchKernelGGL(k_cols_fill<TIn>, dim3((unsigned)((h->L / 4 + 255) / 256), (unsigned)nc), dim3(256), 0, h->stream, h->pm->tiles, (const TIn *)d_g,
                           (long long)N, (long long)ld, (long long)(col0 + c0), (int)h->plan.R, (int)h->plan.S, (const double *)d_mu,
                           (const double *)h->cm.d_rs);
        e = hipStreamSynchronize(h->stream);  // the staging buffer is reused by the next chunk
    }
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("panel columns: ") + hipGetErrorString(e));
    REQUIRE(bad == 0u, NGP_ERR_ARG, "non-finite genotype value in panel");
    return NGP_OK;
}

int end_panel(ngp_handle *h) {
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->panel_open && h->pm, NGP_ERR_STATE, "no open panel (ngp_begin_panel)");
    h->panel_open = false;
    return build_gram(h);
}

template <typename TIn>
int set_panel_host(ngp_handle *h, const TIn *M, int64_t N, int64_t P, int64_t ld, int centre) {
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(M != nullptr, NGP_ERR_ARG, "null panel pointer");
    REQUIRE(ld >= N, NGP_ERR_ARG, "leading dimension smaller than N");
    if ((rc = begin_panel(h, N, P))) return rc;
    if ((rc = panel_columns<TIn>(h, 0, M, P, ld, centre))) return rc;
    return end_panel(h);
}

// does any block of this model take the inverse form?  (a BayesPR set must exist: blocks without an owner are all zeros either way)
bool wants_tinv(const ngp_handle *h) {
    if (h->chain_form != 1) return false;
    for (const HSet &st : h->sets)
        if (st.method == NGP_METHOD_BAYESPR || st.method == NGP_METHOD_BAYESLV || st.method == NGP_METHOD_TUPLE) return true;
    return false;
}

// Which blocks are linear (every lane BayesPR, unowned or -- in a fine-seam call, active_set >= 0 -- of another set than the sampled
// one: those lanes are inactive): their chain takes the inverse form (k_tinv).  Static for a model; the table goes to the device when
// the model or the active set changed.  A Tuple set owns its blocks to the end of the last one (ncol = its span).
int sync_linear_blocks(ngp_handle *h, int active_set) {
    // (the flags are cleared: the key goes stale with them, or a later call under form 1 would find it matching and keep them zero)
    if (!wants_tinv(h) || h->cm.tinv_blocks != h->NBLK) { h->cm.lin_all = 0; h->cm.lin_any = 0; h->cm.blin_for = -2; return NGP_OK; }
    if (h->cm.blin_for == active_set) return NGP_OK;
    // 1 = BayesPR / unowned / inactive lanes only; 1 + k = a block of a k-set Tuple (its chain is linear too: one step per locus);
    // 0 = a lane of BayesB / BayesC / BayesR: the step chains
    std::vector<unsigned> bl((size_t)h->NBLK, 1u);
    for (size_t si = 0; si < h->sets.size(); si++) {
        const HSet &st = h->sets[si];
        if (st.method == NGP_METHOD_BAYESPR || st.method == NGP_METHOD_BAYESLV || (active_set >= 0 && (int)si != active_set)) continue;
        const unsigned code = (st.method == NGP_METHOD_TUPLE) ? 1u + (unsigned)st.tk : 0u;
        for (int64_t t = st.col0 / NGP_BLK; t <= (st.col0 + st.ncol - 1) / NGP_BLK && t < h->NBLK; t++) bl[(size_t)t] = code;
    }
    int64_t n1 = 0, nany = 0;
    for (unsigned v : bl) { n1 += (v == 1u); nany += (v != 0u); }
    h->cm.lin_all = (n1 == h->NBLK) ? 1 : 0;
    h->cm.lin_any = (nany > 0) ? 1 : 0;
    HCHK(hipMemcpyAsync(h->cm.d_blin, bl.data(), (size_t)h->NBLK * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
    HCHK(hipStreamSynchronize(h->stream));  // (bl is a local)
    h->cm.blin_for = active_set;
    return NGP_OK;
}

int sync_tables(ngp_handle *h) {
    int rc;
    if (wants_tinv(h) && h->cm.tinv_blocks != h->NBLK) {
        if ((rc = h->cm.d_tinv.alloc(h, (size_t)h->NBLK * NGP_BLK * NGP_BLK))) return rc;
        if ((rc = h->cm.d_blin.alloc(h, (size_t)h->NBLK))) return rc;
        h->cm.tinv_blocks = h->NBLK;
        h->cm.blin_for = -2;
    }
    if (h->tables_dirty) h->cm.blin_for = -2;
    if (!h->tables_dirty) return NGP_OK;
    const size_t pp = (size_t)h->Ppad;
    HCHK(hipMemcpy(h->cm.d_setof, h->h_setof.data(), pp, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(h->cm.d_loc, h->h_loc.data(), pp * sizeof(int32_t), hipMemcpyHostToDevice));
    HCHK(hipMemcpy(h->cm.d_vbidx, h->h_vbidx.data(), pp * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = h->mm.d_regs.alloc(h, h->h_regs.size()))) return rc;
    if ((rc = h->mm.d_seg_k0.alloc(h, h->h_seg_k0.size()))) return rc;
    if ((rc = h->mm.d_seg_len.alloc(h, h->h_seg_len.size()))) return rc;
    if ((rc = h->mm.d_segpart.alloc(h, h->h_seg_k0.size()))) return rc;
    if ((rc = h->mm.d_seg_set.alloc(h, h->h_seg_set.size()))) return rc;
    if ((rc = h->mm.d_regchi.alloc(h, h->h_regs.size()))) return rc;
    if (!h->h_regs.empty()) {
        HCHK(hipMemcpy(h->mm.d_regs, h->h_regs.data(), h->h_regs.size() * sizeof(DReg), hipMemcpyHostToDevice));
        HCHK(hipMemcpy(h->mm.d_seg_k0, h->h_seg_k0.data(), h->h_seg_k0.size() * sizeof(long long), hipMemcpyHostToDevice));
        HCHK(hipMemcpy(h->mm.d_seg_len, h->h_seg_len.data(), h->h_seg_len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HCHK(hipMemcpy(h->mm.d_seg_set, h->h_seg_set.data(), h->h_seg_set.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (!h->h_tregs.empty()) {
        if ((rc = h->mm.d_tregs.alloc(h, h->h_tregs.size()))) return rc;
        if ((rc = h->mm.d_tseg_l0.alloc(h, h->h_tseg_l0.size()))) return rc;
        if ((rc = h->mm.d_tseg_len.alloc(h, h->h_tseg_len.size()))) return rc;
        if ((rc = h->mm.d_tseg_set.alloc(h, h->h_tseg_set.size()))) return rc;
        if ((rc = h->mm.d_tsegpart.alloc(h, h->h_tseg_l0.size() * NGP_TPAIRS))) return rc;
        HCHK(hipMemcpy(h->mm.d_tregs, h->h_tregs.data(), h->h_tregs.size() * sizeof(DTReg), hipMemcpyHostToDevice));
        HCHK(hipMemcpy(h->mm.d_tseg_l0, h->h_tseg_l0.data(), h->h_tseg_l0.size() * sizeof(long long), hipMemcpyHostToDevice));
        HCHK(hipMemcpy(h->mm.d_tseg_len, h->h_tseg_len.data(), h->h_tseg_len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HCHK(hipMemcpy(h->mm.d_tseg_set, h->h_tseg_set.data(), h->h_tseg_set.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    h->tables_dirty = false;
    return NGP_OK;
}

bool is_kept(const ngp_handle *h, int64_t it) {  // src/samplers.jl:26
    if (it < h->burnIn + h->thin || it > h->chainLength) return false;
    return ((it - h->burnIn) % h->thin) == 0;
}

// Direct quads (role_streamer_rows): the row waves of the row-owning streamer over fp32 tiles load the last NGP_ROWS_DIRECT quads of
// their GEMV chains themselves, and the loader wave requests that much less through its LDS-DMA queue.  One shard per workgroup, the
// loader's early part [0, H) untouched (NQ - 7 KD >= H), and only from shards of NGP_DIRECT_MIN_R rows on.  Knob bit 15 (timing only)
// withholds them, bit 16 (timing and tests) offers them at any height the early part allows.  The values and their order do not change.
static bool sweep_direct_quads(const ngp_handle *h) {
    const int nq = (int)h->plan.R / 4, hq = std::min<int>(NGP_ROWS_HMAX, (nq + 1) / 2);
    return h->plan.mode == 1 && h->plan.streamer == 2 && h->plan.V == 1 && h->req.storage == 0 && !(h->knob & NGP_KNOB_NO_DIRECT) &&
           nq - NGP_ROWS_NW * NGP_ROWS_DIRECT >= hq && (h->plan.R >= NGP_DIRECT_MIN_R || (h->knob & NGP_KNOB_DIRECT_ANY_R));
}

// launch arguments of the persistent sweep over blocks [tb0, tb1) of this handle's chain (advances the launch nonce)
void fill_sweep_args(ngp_handle *h, int64_t tb0, int64_t tb1, SweepArgs &A) {
    const int R = (int)h->plan.R, S = (int)h->plan.S;
    A.tiles = h->pm->tiles; A.ycorr = h->cm.d_ycorr; A.gramx = h->pm->gramx;
    const bool tf = wants_tinv(h) && h->cm.tinv_blocks == h->NBLK;
    A.tinv = (tf && h->cm.lin_any) ? h->cm.d_tinv : nullptr;
    A.blin = (tf && h->cm.lin_any) ? h->cm.d_blin : nullptr;
    A.lin_all = (tf && h->cm.lin_any) ? h->cm.lin_all : 0;
    A.V = h->plan.V; A.D = h->plan.D; A.R = R; A.S = S; A.NG = h->plan.NG; A.near = h->plan.near; A.fine_ok = 0; A.t0 = (int)tb0; A.t1 = (int)tb1;
    A.beta = h->cm.d_beta; A.delta = h->cm.d_delta; A.c = h->cm.d_c; A.w = h->cm.d_w; A.q = h->cm.d_q; A.mpm = h->pm->mpm; A.chi = h->cm.d_chi;
    A.setof = h->cm.d_setof; A.vbidx = h->cm.d_vbidx; A.sets = h->cm.d_sets; A.varBeta = h->mm.d_varBeta;
    A.rcls = h->mm.d_rcls; A.rhs0 = h->cm.d_rhs0; A.scal = h->cm.d_scal; A.Ppad = h->Ppad;
    A.tup = h->ntuple ? h->mm.d_tup : nullptr; A.tupc = h->mm.d_tupc; A.tupg = h->mm.d_tupg;
    A.acc = (unsigned long long *)h->cm.d_ccnt.get(); A.dlt = h->cm.d_cdlt; A.dltg = h->cm.d_cdltg;
    h->launch_seq = (h->launch_seq % 4095u) + 1u;  // 1..4095: never the zero the ring is born with
    A.nonce = h->launch_seq;
    A.flag_dlt = h->cm.d_ccnt + (size_t)NGP_RING * NGP_FX_COPIES * NGP_BLK * 2; A.abort_w = h->cm.d_abort; A.xcc_w = h->cm.d_abort + 16;
    A.census = (h->dbg_mode == 0) ? h->cm.d_ccnt + h->cm.census_off : nullptr;  // timing modes leave roles out: no census there
    A.census_tbl = h->cm.d_census_tbl; A.iter_tag = (unsigned)(h->iter + 1);
    A.census_fail = (h->dbg_census_fail_iter > 0 && !h->exclusive) ? (unsigned)h->dbg_census_fail_iter : 0u;
    A.dbg = h->hm.d_dbg;
    A.fine_ok = (streamer_lds(h->plan, 1) + 8192 <= sweep_lds(h->plan, SweepKernel::diag)) ? 1 : 0;  // diagnostic timeline fits in LDS
    // workgroup NG is a warmer candidate (role_warmer): one shard per streamer workgroup, its reducer without a far lag, and NG a multiple
    // of eight, so that round-robin placement puts it on the sampler's XCD (the kernel reads the XCC ids; the fused and tall kernels ignore the bit)
    // Not in a timing mode (ngp_debug_set_mode): those leave roles out -- no sampler whose word the warmer could read, no dlt to pace it -- and
    // keep measuring the streamers as they always did; with knob bit 11 they show the streamers a warmer has relieved.
    // Only beside the row-owning streamer over fp32 tiles, where the loaders' stream bounds the sweep: measured with the warmer, the phase
    // streamer at 10k x 100k (160 KB of planes per 1.8-us block are more than one CU pulls) lost 22 %, byte tiles at 50k x 600k 1.3 %
    // ("The warmer"; profiles/warm_helper_bench.json).  Knob bit 13 (timing only) withholds the role.
    // And only from shards of 160 rows on: below, the sampler bounds the sweep, the loaders have time to spare, and one CU's warming reaches
    // the L2 later than thirty loaders' (measured: R = 68 and 116 lose 1-3 % with the warmer, R = 164 gains 3 %, 196 9 %, 204 7.6 %).
    // Knob bit 14 (timing only, the tests' way to the role at short shards) offers it at any height.
    const bool warmer_tall = h->plan.R >= NGP_WARMER_MIN_R || (h->knob & NGP_KNOB_WARMER_ANY_R);
    const bool warmer_idle = h->plan.NG > 0 && h->plan.NG % 8 == 0 && h->plan.near + h->plan.NG >= h->plan.D;
    const bool warmer = h->dbg_mode == 0 && h->plan.streamer == 2 && h->plan.V == 1 && !(h->knob & NGP_KNOB_NO_WARMER) &&
                        warmer_tall && warmer_idle;
    A.variant = h->plan.streamer; A.knob = (h->knob & ~(NGP_KNOB_WARMER | NGP_KNOB_DIRECT)) | (warmer ? NGP_KNOB_WARMER : 0) | (sweep_direct_quads(h) ? NGP_KNOB_DIRECT : 0);
    A.mean = h->pm->mean; A.N = h->N;
    A.dbg_mode = h->dbg_mode;
}

// one sweep over blocks [tb0, tb1): persistent kernel (mode 1) or two launches per block (mode 0)
void launch_sweep(ngp_handle *h, int64_t tb0, int64_t tb1, hipEvent_t *evs) {
    const int R = (int)h->plan.R, S = (int)h->plan.S;
    if (h->plan.mode == 1) {
        // (the hand-off counters were zeroed by k_prep, which precedes every sweep in the stream)
        SweepArgs A;
        fill_sweep_args(h, tb0, tb1, A);
        SweepKernel k = pick_kernel(h->plan, 1, h->hm.d_dbg || h->dbg_mode, h->ntuple > 0, h->nclass_total > 0, !h->mm.rc.empty());
        // the direct quads exist in two instantiations: k_sweep_dq, which takes the lean kernel's place, and the diagnostic kernel
        if (k == SweepKernel::lean && (A.knob & NGP_KNOB_DIRECT)) k = SweepKernel::lean_dq;
        else if (k != SweepKernel::diag) A.knob &= ~NGP_KNOB_DIRECT;
        h->last_grid = sweep_grid(h->plan);
        if (evs) (void)hipEventRecord(evs[0], h->stream);
        launch_sweep_kernel(k, h->last_grid, sweep_lds(h->plan, k), h->stream, &A);
        if (evs) (void)hipEventRecord(evs[1], h->stream);
        h->sweep_launches += 1;
        return;
    }
    int e = 0;
    for (int64_t t = tb0; t <= tb1; t++) {
        const int do_upd = t > tb0, do_gemv = t < tb1;
        if (evs && do_gemv) (void)hipEventRecord(evs[e++], h->stream);
        hipLaunchKernelGGL(k_step, dim3((unsigned)S), dim3(256), h->lds_step, h->stream, h->pm->tiles, h->cm.d_ycorr, h->cm.d_dlt, h->cm.d_part, R,
                           S, (int)t, do_upd, do_gemv);
        if (evs && do_gemv) (void)hipEventRecord(evs[e++], h->stream);
        if (do_gemv)
            hipLaunchKernelGGL(h->mm.rc.empty() ? k_recur<false> : k_recur<true>, dim3(1), dim3(256), 0, h->stream, h->cm.d_part, h->pm->gramx, h->plan.D, S, (int)t, h->cm.d_beta, h->cm.d_delta,
                               h->cm.d_c, h->cm.d_w, h->cm.d_q, h->pm->mpm, h->cm.d_chi, h->cm.d_setof, h->cm.d_vbidx, h->cm.d_sets, h->mm.d_varBeta, h->cm.d_dlt, h->mm.d_rcls,
                               (long long)h->Ppad, h->cm.d_rhs0, h->cm.d_scal, h->mm.d_tup, h->mm.d_tupc, h->mm.d_tupg,
                               (const double *)((wants_tinv(h) && h->cm.tinv_blocks == h->NBLK && h->cm.lin_any) ? h->cm.d_tinv : nullptr), (const unsigned *)h->cm.d_blin);
    }
    h->sweep_launches += 2 * (tb1 - tb0) + 1;
}

// placement census of the last sweep launch (SweepArgs.census_tbl): who arrived, and where
std::string census_report(ngp_handle *h) {
    const size_t grid = (size_t)(h->last_grid > 0 ? h->last_grid : sweep_grid(h->plan));
    std::vector<unsigned long long> tb(grid, 0ull);
    if (!h->cm.d_census_tbl || hipMemcpy(tb.data(), h->cm.d_census_tbl, grid * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return "(no census)";
    int per_xcc[16] = {0}, per_se[16][8] = {{0}};
    size_t arrived = 0;
    std::string missing;
    for (size_t b = 0; b < grid; b++) {
        if (tb[b] == 0ull) { if (missing.size() < 120) missing += (missing.empty() ? "" : ",") + std::to_string(b); continue; }
        arrived++;
        const unsigned x = ((unsigned)(tb[b] >> 32) - 1u) & 15u, hw = (unsigned)tb[b];
        per_xcc[x]++; per_se[x][(hw >> 13) & 7u]++;  // HW_REG_HW_ID: cu_id [11:8], sh_id [12], se_id [15:13]
    }
    std::string r = std::to_string(arrived) + " of " + std::to_string(grid) + " workgroups resident; per XCD";
    for (int x = 0; x < 8; x++) {
        r += " " + std::to_string(per_xcc[x]) + "(";
        for (int e = 0; e < 4; e++) r += (e ? "/" : "") + std::to_string(per_se[x][e]);
        r += ")";
    }
    if (!missing.empty()) r += "; missing blocks " + missing;
    return r;
}

// status of the sweeps launched so far: NGP_OK, NGP_RETRY_CENSUS (a launch ended at its census with nothing changed: *iter_failed
// says which iteration; the abort words are cleared, the caller runs it again with the device to itself) or an error (poisoned)
#define NGP_RETRY_CENSUS 1
int check_abort(ngp_handle *h, int64_t *iter_failed = nullptr) {
    if (h->plan.mode != 1 && !h->cm.gv.on) return NGP_OK;  // (the per-block engine raises no abort word; the variance pass may)
    unsigned w[2] = {0, 0};
    HCHK(hipMemcpy(w, h->cm.d_abort, sizeof(w), hipMemcpyDeviceToHost));
    if (w[0] == 0) return NGP_OK;
    (void)hipMemset(h->cm.d_abort, 0, sizeof(w));
    if (w[0] == NGP_ABORT_CENSUS && iter_failed && !h->exclusive) {
        // iter_tag holds the low 32 bits of the iteration: the launches in flight are at most 16 iterations ahead of it
        const int64_t base = (h->iter + 1) & ~(int64_t)0xFFFFFFFF;
        int64_t it = base | (int64_t)w[1];
        if (it > h->iter + 1) it -= ((int64_t)1 << 32);
        *iter_failed = it;
        return NGP_RETRY_CENSUS;
    }
    h->poisoned = true;  // ycorr / beta were left half-way through a sweep (or a grid was not resident even alone on the device)
    if (w[0] == NGP_ABORT_CENSUS)
        return fail(h, NGP_ERR_HIP, "persistent sweep: the grid did not become resident although this call had leased the whole device (" +
                                        census_report(h) + "): another process holding CUs?  The chain state is invalid until ngp_set_y / ngp_set_state");
    if (w[0] == NGP_ABORT_GENVAR)
        return fail(h, NGP_ERR_HIP, "genomic variance: a term left the fixed-point range of its sum (non-finite effects?); the pass and every kernel "
                                    "behind it that reads the abort word returned at once: the variance sums and the chain state are invalid until "
                                    "ngp_set_y / ngp_set_state");
    if (w[0] == 7u)  // NGP_ABORT_FX
        return fail(h, NGP_ERR_HIP, "persistent sweep: a partial dot product left the fixed-point range of its accumulator (non-finite residual or effects, "
                                    "or within one iteration the residual grew more than 32-fold over the larger of its norm at the head and "
                                    "sqrt(W varE) / 16, W the number of records or the sum of their weights); the chain state is invalid until "
                                    "ngp_set_y / ngp_set_state");
    return fail(h, NGP_ERR_HIP, "persistent sweep kernel gave up waiting (role code " + std::to_string(w[0]) +
                                    "): workgroups not co-resident (another kernel holding CUs?) or a hand-off was lost; the chain "
                                    "state is invalid until ngp_set_y / ngp_set_state");
}

// the variance model of one BayesLV set on h->stream (ngp_logvar.h): slice draws, c, zeta, varZeta
void launch_lv(ngp_handle *h, HLv &V, uint64_t it) {
    const HSet &hs = h->sets[(size_t)V.set];
    const long long n = (long long)V.n;
    const unsigned gseg = (unsigned)(((n + 255) / 256 + 3) / 4);
    const double *beta = h->cm.d_beta + hs.col0;
    double *vb = h->mm.d_varBeta + hs.vb_off;
    const unsigned *ab = (const unsigned *)h->cm.d_abort;
    hipLaunchKernelGGL(k_lv_slice, dim3(gseg), dim3(256), 0, h->stream, n, V.ncov, beta, vb, (const double *)V.d_zeta, (const double *)V.d_C,
                       (const double *)V.d_st, V.d_logv.get(), V.d_part.get(), V.d_trapseg.get(), V.set, h->seed, (uint64_t)h->chain, it, ab);
    hipLaunchKernelGGL(k_lv_coef, dim3(1), dim3(64), 0, h->stream, n, V.ncov, (const double *)V.d_iCpC, (const double *)V.d_part,
                       (const int *)V.d_trapseg, V.d_st.get(), V.set, h->seed, (uint64_t)h->chain, it, ab);
    hipLaunchKernelGGL(k_lv_resid, dim3(gseg), dim3(256), 0, h->stream, n, V.ncov, (const double *)V.d_C, (const double *)V.d_st,
                       (const double *)V.d_logv, V.d_zeta.get(), V.mode, V.d_vpart.get(), ab);
    if (V.mode == 0) return;
    const double *x = (V.mode == 1) ? V.d_zeta.get() : V.d_logv.get();
    hipLaunchKernelGGL(k_lv_reduce, dim3(1), dim3(64), 0, h->stream, n, 0, V.mode, V.frac, (const double *)V.d_vpart, V.d_st.get(), ab);
    hipLaunchKernelGGL(k_lv_ssq, dim3(gseg), dim3(256), 0, h->stream, n, x, (const double *)V.d_st, V.d_vpart.get(), ab);
    hipLaunchKernelGGL(k_lv_reduce, dim3(1), dim3(64), 0, h->stream, n, 1, V.mode, V.frac, (const double *)V.d_vpart, V.d_st.get(), ab);
}

void launch_variance(ngp_handle *h, int active_set, uint64_t it) {
    for (auto &V : h->mm.lv)  // BayesLV sets: their variance model instead of a region draw (src/functions.jl:442-485)
        if (active_set < 0 || V.set == active_set) launch_lv(h, V, it);
    const long long nseg = (long long)h->h_seg_k0.size(), nreg = (long long)h->h_regs.size();
    if (nseg > 0) {
        hipLaunchKernelGGL(k_regssq, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, h->stream, nseg, h->mm.d_seg_k0, h->mm.d_seg_len,
                           h->cm.d_beta, h->mm.d_segpart, h->cm.d_abort);
        if (h->nclass_total > 0)
            hipLaunchKernelGGL(k_rssq, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, h->stream, nseg, h->mm.d_seg_k0, h->mm.d_seg_len, h->mm.d_seg_set,
                               h->cm.d_sets, h->cm.d_beta, h->cm.d_delta, h->mm.d_segpart, h->cm.d_abort);
        hipLaunchKernelGGL(k_regdraw, dim3((unsigned)((nreg + 63) / 64)), dim3(64), 0, h->stream, nreg, h->mm.d_regs, h->mm.d_segpart,
                           h->cm.d_sets, h->mm.d_varBeta, active_set, h->mm.d_regchi, h->seed, (uint64_t)h->chain, it, h->cm.d_abort);
    }
    if (!h->h_tregs.empty()) {  // Tuple sets: Sb = B_r'B_r per region, then the inverse-Wishart draw of its variance matrix
        const long long ntseg = (long long)h->h_tseg_l0.size(), ntreg = (long long)h->h_tregs.size();
        hipLaunchKernelGGL(k_tuple_ssq, dim3((unsigned)((ntseg + 3) / 4)), dim3(256), 0, h->stream, ntseg, h->mm.d_tseg_l0, h->mm.d_tseg_len, h->mm.d_tseg_set,
                           h->mm.d_tup, h->cm.d_beta, h->mm.d_tsegpart, h->cm.d_abort);
        hipLaunchKernelGGL(k_tuple_draw, dim3((unsigned)((ntreg + 63) / 64)), dim3(64), 0, h->stream, ntreg, h->mm.d_tregs, h->mm.d_tsegpart, h->mm.d_tup,
                           h->mm.d_varBeta, active_set, h->seed, (uint64_t)h->chain, it, h->cm.d_abort);
    }
    hipLaunchKernelGGL(k_pidraw, dim3(1), dim3(64), 0, h->stream, (int)h->sets.size(), h->cm.d_sets, active_set, h->seed,
                       (uint64_t)h->chain, it, h->cm.d_abort);
    for (auto &Rc : h->mm.rc) {  // BayesRCpi sets: class / annotation of every locus, the A variances, pi, annotProb (ngp_bayesrc.h)
        if (active_set >= 0 && Rc.set != active_set) continue;
        const DRc R = Rc.dev();
        const unsigned *ab = (const unsigned *)h->cm.d_abort;
        hipLaunchKernelGGL(k_rc_count, dim3((unsigned)((Rc.nseg + 3) / 4)), dim3(256), 0, h->stream, (const DSet *)h->cm.d_sets, Rc.set, R,
                           (const double *)h->cm.d_beta, h->cm.d_delta.get(), ab);
        hipLaunchKernelGGL(k_rc_draw, dim3(1), dim3(64), 0, h->stream, h->cm.d_sets.get(), Rc.set, R, h->mm.d_varBeta + h->sets[(size_t)Rc.set].vb_off,
                           h->seed, (uint64_t)h->chain, it, ab);
        hipLaunchKernelGGL(k_rc_annot, dim3((unsigned)((Rc.n + 255) / 256)), dim3(256), 0, h->stream, (const DSet *)h->cm.d_sets, Rc.set, R, h->seed,
                           (uint64_t)h->chain, it, ab);
    }
}

// resume_mid: the head of this iteration (varE, intercept, fixed-effect sets) has run already -- its sweep ended at the census
// with nothing changed and is launched again, k_prep first (it redraws the same keyed numbers and clears the hand-off counters)
int sample_enqueue(ngp_handle *h);  // (below)
void launch_diag(ngp_handle *h);    // (below)

// T = inv(L) of every linear block from this iteration's coefficients (k_tinv; behind k_prep in the stream, in front of the sweep)
void launch_tinv(ngp_handle *h) {  // (sync_linear_blocks has run for this call's active set)
    if (!wants_tinv(h) || h->cm.tinv_blocks != h->NBLK || !h->cm.lin_any) return;
    hipLaunchKernelGGL(k_tinv, dim3((unsigned)h->NBLK), dim3(64), 0, h->stream, (const double *)h->pm->gramx, h->plan.D, (const double *)h->cm.d_c,
                       (const unsigned *)h->cm.d_blin, h->cm.d_tinv, (const unsigned *)h->cm.d_abort, (const double *)h->mm.d_tupc, (long long)h->Ppad);
}

// one random-effect set on h->stream (ngp_random.h): level sums and draws, Gauss-Seidel for a general K, ycorr update, varU
void launch_random(ngp_handle *h, int r, uint64_t it) {
    HRand &R = h->mm.rnd[(size_t)r];
    const long long q = (long long)R.q;
    if (R.tk > 1) {  // a correlated (Tuple) set: ngp_random_tuple.h
        const int k = R.tk;
        const unsigned *ab = (const unsigned *)h->cm.d_abort;
        const DScal *sc = (const DScal *)h->cm.d_scal;
        const long long *kp = R.d_kptr, *wp = R.d_wptr;
        const int *kc = R.d_kcol, *wc = R.d_wcol;
        const double *kv = R.d_kval, *wv = R.d_wval;
        const TupScr T = tup_scr(R.d_scr.get(), q, k);
        hipLaunchKernelGGL(k_tup_prep, dim3(1), dim3(64), 0, h->stream, k, (const double *)R.d_vu, T.sig, ab);
        const int lpb = 4 / k;
        hipLaunchKernelGGL(k_tup_levels, dim3((unsigned)((q + lpb - 1) / lpb)), dim3(256), 0, h->stream, (const double *)h->cm.d_ycorr, (const double *)h->cm.d_rs, q,
                           k, (const long long *)R.d_lptr, (const int *)R.d_lrows, (const double *)R.d_wd, (const double *)R.d_kdiag, kp, kc, kv,
                           (const double *)R.d_u, R.d_scr.get(), sc, r, h->seed, (uint64_t)h->chain, it, ab);
        if (R.scheduled()) {  // the level schedule: one launch per wide depth, one per run of narrow depths, in depth order
            for (const HRand::Launch &pl : R.plan) {
                if (pl.wide)
                    hipLaunchKernelGGL(k_tup_sched_wide, dim3((unsigned)((pl.r1 - pl.r0 + 255) / 256)), dim3(256), 0, h->stream, q, k, kp, kc, kv, wp, wc, wv,
                                       R.d_u.get(), R.d_scr.get(), sc, (const int *)R.d_order, pl.r0, pl.r1, ab);
                else
                    hipLaunchKernelGGL(k_tup_sched_fused, dim3(1), dim3(1024), 0, h->stream, q, k, kp, kc, kv, wp, wc, wv, R.d_u.get(), R.d_scr.get(), sc,
                                       (const int *)R.d_order, (const long long *)R.d_dptr, pl.d0, pl.d1, ab);
            }
        } else {
            const size_t ub = (size_t)q * (size_t)k * sizeof(double);
            const int use_lds = ub <= NGP_LDS_MAX;
            hipLaunchKernelGGL(k_tup_gs, dim3(1), dim3(64), use_lds ? ub : 0, h->stream, q, k, kp, kc, kv, wp, wc, wv, R.d_u.get(), R.d_scr.get(), sc, use_lds, ab);
        }
        hipLaunchKernelGGL(k_tup_update, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, h->cm.d_ycorr, (const double *)h->cm.d_rs, (long long)h->N, k,
                           (const int *)R.d_level, (const double *)T.du, ab);
        hipLaunchKernelGGL(k_tup_var, dim3(1), dim3(1024), 0, h->stream, q, k, kp, kc, kv, (const double *)R.d_u, R.d_vu.get(), R.df, (const double *)R.d_scaleM, r,
                           h->seed, (uint64_t)h->chain, it, ab);
        return;
    }
    if (R.hyb) {  // sparse S plus a dense trailing block (ngp_hybrid.h): the CSR engine over the head rows, the seed, the blocked engine over T
        const long long hd = (long long)R.hd, nd = q - hd, ld = (long long)R.dk->ld;
        const double *T = R.dk->K;
        const unsigned *ab = (const unsigned *)h->cm.d_abort;
        const long long *kp = R.d_kptr;
        const int *kc = R.d_kcol;
        const double *kv = R.d_kval;
        hipLaunchKernelGGL(k_rand_levels, dim3((unsigned)((q + 3) / 4)), dim3(256), 0, h->stream, (const double *)h->cm.d_ycorr, (const double *)h->cm.d_rs, q,
                           (const long long *)R.d_lptr, (const int *)R.d_lrows, (const double *)R.d_zpz, (const double *)R.d_kdiag, kp, kc, kv, R.d_u,
                           (const double *)R.d_vu, R.d_scr, 1, (const DScal *)h->cm.d_scal, r, h->seed, (uint64_t)h->chain, it, ab);
        hipLaunchKernelGGL(k_hyb_dhi, dim3((unsigned)((nd + 3) / 4)), dim3(256), 0, h->stream, T, ld, nd, (const double *)(R.d_u + hd), R.d_scr + hd, q, ab);
        if (hd > 0 && R.scheduled()) {  // the level schedule of the head rows, as a CSR set runs it (q: the stride of the scratch rows)
            for (const HRand::Launch &pl : R.plan) {
                if (pl.wide)
                    hipLaunchKernelGGL(k_rand_sched_wide, dim3((unsigned)((pl.r1 - pl.r0 + 255) / 256)), dim3(256), 0, h->stream, q, kp, kc, kv, R.d_u.get(),
                                       (const double *)R.d_vu, R.d_scr.get(), (const int *)R.d_order, pl.r0, pl.r1, ab);
                else
                    hipLaunchKernelGGL(k_rand_sched_fused, dim3(1), dim3(1024), 0, h->stream, q, kp, kc, kv, R.d_u.get(), (const double *)R.d_vu,
                                       R.d_scr.get(), (const int *)R.d_order, (const long long *)R.d_dptr, pl.d0, pl.d1, ab);
            }
        } else if (hd > 0) {
            hipLaunchKernelGGL(k_hyb_gs, dim3(1), dim3(64), 0, h->stream, hd, q, kp, kc, kv, R.d_u.get(), (const double *)R.d_vu, R.d_scr.get(), ab);
        }
        hipLaunchKernelGGL(k_hyb_seed, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, h->stream, hd, q, kp, kc, kv, (const double *)R.d_u, R.d_scr, ab);
        for (long long t = 0; t * 64 < nd; t++) {
            const long long below = nd - 64 * t - 64;
            const unsigned nwg = below > 0 ? (unsigned)((below + NGP_DENSE_WG_ROWS - 1) / NGP_DENSE_WG_ROWS) : 1u;
            hipLaunchKernelGGL(k_hyb_block, dim3(nwg), dim3(256), 0, h->stream, T, ld, nd, (int)t, R.d_u + hd, (const double *)R.d_vu, R.d_scr + hd, q, ab);
        }
        hipLaunchKernelGGL(k_rand_update, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, h->cm.d_ycorr, (const double *)h->cm.d_rs, (long long)h->N,
                           (const int *)R.d_level, (const double *)(R.d_scr + NGP_RS_DU * q), ab);
        hipLaunchKernelGGL(k_hyb_var, dim3(1), dim3(1024), 0, h->stream, q, hd, kp, kc, kv, (const double *)R.d_kdiag, (const double *)R.d_u,
                           (const double *)R.d_scr, R.d_vu, R.df, R.sdf, r, h->seed, (uint64_t)h->chain, it, ab);
        return;
    }
    if (R.dk) {  // dense K: the blocked engine (ngp_dense.h), one launch per block of 64 levels between the level terms and the ycorr update
        const double *K = R.dk->K;
        const long long ld = (long long)R.dk->ld;
        const unsigned *ab = (const unsigned *)h->cm.d_abort;
        hipLaunchKernelGGL(k_rand_levels, dim3((unsigned)((q + 3) / 4)), dim3(256), 0, h->stream, (const double *)h->cm.d_ycorr, (const double *)h->cm.d_rs, q,
                           (const long long *)R.d_lptr, (const int *)R.d_lrows, (const double *)R.d_zpz, (const double *)R.d_kdiag,
                           (const long long *)nullptr, (const int *)nullptr, (const double *)nullptr, R.d_u, (const double *)R.d_vu, R.d_scr, 1,
                           (const DScal *)h->cm.d_scal, r, h->seed, (uint64_t)h->chain, it, ab);
        hipLaunchKernelGGL(k_dense_dhi, dim3((unsigned)((q + 3) / 4)), dim3(256), 0, h->stream, K, ld, q, (const double *)R.d_u, R.d_scr, ab);
        for (long long t = 0; t * 64 < q; t++) {
            const long long below = q - 64 * t - 64;
            const unsigned nwg = below > 0 ? (unsigned)((below + NGP_DENSE_WG_ROWS - 1) / NGP_DENSE_WG_ROWS) : 1u;
            hipLaunchKernelGGL(k_dense_block, dim3(nwg), dim3(256), 0, h->stream, K, ld, q, (int)t, R.d_u, (const double *)R.d_vu, R.d_scr, ab);
        }
        hipLaunchKernelGGL(k_rand_update, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, h->cm.d_ycorr, (const double *)h->cm.d_rs, (long long)h->N,
                           (const int *)R.d_level, (const double *)(R.d_scr + NGP_RS_DU * q), ab);
        hipLaunchKernelGGL(k_dense_var, dim3(1), dim3(1024), 0, h->stream, q, (const double *)R.d_kdiag, (const double *)R.d_u, (const double *)R.d_scr, R.d_vu,
                           R.df, R.scale, r, h->seed, (uint64_t)h->chain, it, ab);
        return;
    }
    hipLaunchKernelGGL(k_rand_levels, dim3((unsigned)((q + 3) / 4)), dim3(256), 0, h->stream, (const double *)h->cm.d_ycorr, (const double *)h->cm.d_rs, q,
                       (const long long *)R.d_lptr, (const int *)R.d_lrows, (const double *)R.d_zpz, (const double *)R.d_kdiag,
                       (const long long *)R.d_kptr, (const int *)R.d_kcol, (const double *)R.d_kval, R.d_u, (const double *)R.d_vu, R.d_scr,
                       (int)R.offdiag, (const DScal *)h->cm.d_scal, r, h->seed, (uint64_t)h->chain, it, (const unsigned *)h->cm.d_abort);
    if (R.offdiag && R.scheduled()) {  // the level schedule: one launch per wide depth, one per run of narrow depths, in depth order
        for (const HRand::Launch &pl : R.plan) {
            if (pl.wide)
                hipLaunchKernelGGL(k_rand_sched_wide, dim3((unsigned)((pl.r1 - pl.r0 + 255) / 256)), dim3(256), 0, h->stream, q, (const long long *)R.d_kptr,
                                   (const int *)R.d_kcol, (const double *)R.d_kval, R.d_u.get(), (const double *)R.d_vu, R.d_scr.get(), (const int *)R.d_order,
                                   pl.r0, pl.r1, (const unsigned *)h->cm.d_abort);
            else
                hipLaunchKernelGGL(k_rand_sched_fused, dim3(1), dim3(1024), 0, h->stream, q, (const long long *)R.d_kptr, (const int *)R.d_kcol,
                                   (const double *)R.d_kval, R.d_u.get(), (const double *)R.d_vu, R.d_scr.get(), (const int *)R.d_order,
                                   (const long long *)R.d_dptr, pl.d0, pl.d1, (const unsigned *)h->cm.d_abort);
        }
    } else if (R.offdiag) {
        const int use_lds = (size_t)q * sizeof(double) <= NGP_LDS_MAX;
        hipLaunchKernelGGL(k_rand_gs, dim3(1), dim3(64), use_lds ? (size_t)q * sizeof(double) : 0, h->stream, q, (const long long *)R.d_kptr,
                           (const int *)R.d_kcol, (const double *)R.d_kval, R.d_u, (const double *)R.d_vu, R.d_scr, use_lds, (const unsigned *)h->cm.d_abort);
    }
    hipLaunchKernelGGL(k_rand_update, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, h->cm.d_ycorr, (const double *)h->cm.d_rs, (long long)h->N,
                       (const int *)R.d_level, (const double *)(R.d_scr + NGP_RS_DU * q), (const unsigned *)h->cm.d_abort);
    hipLaunchKernelGGL(k_rand_var, dim3(1), dim3(1024), 0, h->stream, q, (const long long *)R.d_kptr, (const int *)R.d_kcol, (const double *)R.d_kval,
                       (const double *)R.d_u, R.d_vu, R.df, R.sdf, r, h->seed, (uint64_t)h->chain, it, (const unsigned *)h->cm.d_abort);
}

/* ---- prediction: g = X_new beta of every kept draw (ngp_predict.h) ---- */

// does a kept iteration of this chain predict?  (a finished prediction panel beside its training panel, and marker sets to predict from)
bool predicts(const ngp_handle *h) {
    return h->pm && h->pm->pred && h->pm->pred->done && !h->records_only && h->cm.pred_for == h->pm->pred->id && h->cm.pred_rows > 0;
}

// the work items of a chain: every marker set in chunks of NGP_PRED_CB blocks counted from the set's first block
std::vector<PredItem> build_pred_items(const ngp_handle *h, std::vector<int> *set0) {
    std::vector<PredItem> items;
    set0->assign(1, 0);
    for (size_t s = 0; s < h->sets.size(); s++) {
        const HSet &st = h->sets[s];
        const int64_t j0 = st.col0, j1 = st.col0 + st.ncol, tb0 = j0 / NGP_BLK, tb1 = (j1 + NGP_BLK - 1) / NGP_BLK;
        for (int64_t t = tb0; t < tb1; t += NGP_PRED_CB) {
            const int64_t te = std::min<int64_t>(t + NGP_PRED_CB, tb1);
            items.push_back(PredItem{(int)s, (int)t, (int)te, 0, (long long)std::max<int64_t>(j0, t * NGP_BLK), (long long)std::min<int64_t>(j1, te * NGP_BLK)});
        }
        set0->push_back((int)items.size());
    }
    return items;
}

bool same_pred_items(const ngp_handle *a, const ngp_handle *b) {
    if (a->pm != b->pm || a->sets.size() != b->sets.size()) return false;
    for (size_t s = 0; s < a->sets.size(); s++)
        if (a->sets[s].col0 != b->sets[s].col0 || a->sets[s].ncol != b->sets[s].ncol) return false;
    return true;
}

// The chain's prediction arrays for the panel and the sets it has now: allocated (zeroed) when either changed, zeroed again on request
// (ngp_set_y).  Nothing to do without a finished prediction panel.
int ensure_prediction(ngp_handle *h, bool zero) {
    const PredPanel *pp = (h->pm && h->pm->pred && h->pm->pred->done && !h->records_only) ? h->pm->pred.get() : nullptr;
    ChainMem &c = h->cm;
    if (!pp || h->sets.empty()) { c.pred_for = 0; c.pred_rows = 0; return NGP_OK; }
    const int64_t rows = (int64_t)h->sets.size() + 1, Lp = pp->R * pp->S;
    int rc;
    if (c.pred_for != pp->id || c.pred_rows != rows) {
        c.pred_for = 0; c.pred_rows = 0;
        std::vector<int> set0;
        c.pred_items = build_pred_items(h, &set0);
        const size_t ni = c.pred_items.size();
        if ((rc = c.d_pred_sum.alloc(h, (size_t)rows * pp->Np)) || (rc = c.d_pred_sum2.alloc(h, (size_t)rows * pp->Np)) ||
            (rc = c.d_pred_last.alloc(h, (size_t)rows * pp->Np)) || (rc = c.d_pred_part.alloc(h, ni * (size_t)Lp)) || (rc = c.d_pred_mpart.alloc(h, ni)) ||
            (rc = c.d_pred_items.alloc(h, ni)) || (rc = c.d_pred_set0.alloc(h, set0.size())))
            return rc;
        HCHK(hipMemcpyAsync(c.d_pred_items, c.pred_items.data(), ni * sizeof(PredItem), hipMemcpyHostToDevice, h->stream));
        HCHK(hipMemcpyAsync(c.d_pred_set0, set0.data(), set0.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HCHK(hipStreamSynchronize(h->stream));  // (set0 is a local)
        c.pred_for = pp->id; c.pred_rows = rows;
    } else if (zero) {
        HCHK(hipMemsetAsync(c.d_pred_sum, 0, (size_t)rows * pp->Np * sizeof(double), h->stream));
        HCHK(hipMemsetAsync(c.d_pred_sum2, 0, (size_t)rows * pp->Np * sizeof(double), h->stream));
        HCHK(hipMemsetAsync(c.d_pred_last, 0, (size_t)rows * pp->Np * sizeof(double), h->stream));
    }
    return NGP_OK;
}

// ONE pass over the prediction panel for the n chains hs (they predict and hold their marker sets on the same columns as hs[0]), on
// lead's stream: chunk partials, then every chain's sums.  The panel is read once however many chains there are.
void launch_predict(ngp_handle *lead, ngp_handle **hs, int n) {
    const PredPanel &pp = *lead->pm->pred;
    const ChainMem &c0 = hs[0]->cm;
    PredArgs A;
    std::memset(&A, 0, sizeof A);
    for (int i = 0; i < n; i++) {
        ChainMem &c = hs[i]->cm;
        A.c[i] = PredChain{(const double *)c.d_beta.get(), c.d_pred_part.get(), c.d_pred_mpart.get(), c.d_pred_sum.get(), c.d_pred_sum2.get(), c.d_pred_last.get()};
    }
    const bool u8 = lead->req.storage == 1;
    const unsigned nitems = (unsigned)c0.pred_items.size();
    const size_t lds = predict_lds_bytes((int)pp.R, n, u8);
    const PredItem *items = c0.d_pred_items.get();
    const unsigned *ab = (const unsigned *)lead->cm.d_abort;
#define NGP_PRED_CASE(KK)                                                                                                                     \
    case KK:                                                                                                                                  \
        if (u8) {                                                                                                                             \
            (void)hipFuncSetAttribute((const void *)k_predict<KK, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);               \
            hipLaunchKernelGGL((k_predict<KK, true>), dim3(nitems, (unsigned)pp.S), dim3(256), lds, lead->stream, (const void *)pp.tiles.get(), \
                               (const double *)pp.mean, items, A, (int)pp.R, (int)pp.S, (long long)(pp.R * pp.S), ab);                        \
        } else {                                                                                                                              \
            (void)hipFuncSetAttribute((const void *)k_predict<KK, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);              \
            hipLaunchKernelGGL((k_predict<KK, false>), dim3(nitems, (unsigned)pp.S), dim3(256), lds, lead->stream, (const void *)pp.tiles.get(), \
                               (const double *)pp.mean, items, A, (int)pp.R, (int)pp.S, (long long)(pp.R * pp.S), ab);                        \
        }                                                                                                                                     \
        break;
    switch (n) {
        NGP_PRED_CASE(1) NGP_PRED_CASE(2) NGP_PRED_CASE(3) NGP_PRED_CASE(4) NGP_PRED_CASE(5) NGP_PRED_CASE(6) NGP_PRED_CASE(7) NGP_PRED_CASE(8)
        default: return;
    }
#undef NGP_PRED_CASE
    const dim3 cg((unsigned)((pp.Np + 255) / 256), (unsigned)n);
    const int nsets = (int)hs[0]->sets.size();
    if (u8)
        hipLaunchKernelGGL(k_predict_combine<true>, cg, dim3(256), 0, lead->stream, A, (const int *)c0.d_pred_set0.get(), nsets, (long long)pp.Np,
                           (long long)(pp.R * pp.S), ab);
    else
        hipLaunchKernelGGL(k_predict_combine<false>, cg, dim3(256), 0, lead->stream, A, (const int *)c0.d_pred_set0.get(), nsets, (long long)pp.Np,
                           (long long)(pp.R * pp.S), ab);
    lead->cm.pred_launches += 1;
    lead->cm.pred_served += n;
}

/* ---- genomic variance: var_i (X beta)_i of every kept draw per window, set and in all (ngp_genvar.h) ---- */

// does a kept iteration of this chain run the variance pass?
bool gv_active(const ngp_handle *h) { return h->pm && !h->records_only && h->cm.gv.on && h->cm.gv.built; }

// Segments, items and slots of the chain's sets and windows ("Genomic variance", steps 1 and 4), the device
// arrays sized for them; everything the chain has accumulated is dropped (the arrays come back zeroed).
int build_genvar(ngp_handle *h) {
    GenVar &g = h->cm.gv;
    g.built = false;
    g.segs.clear(); g.items.clear(); g.built_for.clear();
    const size_t nsets = h->sets.size();
    g.win.resize(nsets);
    std::vector<int> set_item0(1, 0), set_seg0(1, 0), slot_seg;
    for (size_t s = 0; s < nsets; s++) {
        const HSet &st = h->sets[s];
        g.built_for.push_back(st.col0); g.built_for.push_back(st.ncol);
        const std::vector<int64_t> &w = g.win[s];
        auto gap = [&](int64_t a, int64_t b) {  // columns [a, b) of the set outside every window, in pieces of NGP_GV_ITEM_COLS
            for (int64_t j = a; j < b; j += NGP_GV_ITEM_COLS)
                g.segs.push_back(GvSeg{(long long)(st.col0 + j), (long long)(st.col0 + std::min<int64_t>(j + NGP_GV_ITEM_COLS, b)), -1, 0});
        };
        int64_t at = 0;
        for (size_t k = 0; k + 1 < w.size(); k += 2) {
            gap(at, w[k]);
            slot_seg.push_back((int)g.segs.size());
            g.segs.push_back(GvSeg{(long long)(st.col0 + w[k]), (long long)(st.col0 + w[k + 1]), (int)slot_seg.size() - 1, 0});
            at = w[k + 1];
        }
        gap(at, st.ncol);
        // items: whole segments, in order, while they fit into NGP_GV_ITEM_COLS columns; a longer window stands alone
        for (int e = set_seg0.back(); e < (int)g.segs.size();) {
            int f = e + 1;
            while (f < (int)g.segs.size() && g.segs[(size_t)f].j1 - g.segs[(size_t)e].j0 <= NGP_GV_ITEM_COLS) f++;
            g.items.push_back(GvItem{(int)s, e, f, 0, g.segs[(size_t)e].j0, g.segs[(size_t)f - 1].j1});
            e = f;
        }
        set_seg0.push_back((int)g.segs.size());
        set_item0.push_back((int)g.items.size());
    }
    g.nwin = (int64_t)slot_seg.size();
    g.nslots = g.nwin + (int64_t)nsets + 1;
    g.ncol_w = (h->L + NGP_GV_ROWS - 1) / NGP_GV_ROWS;  // workgroup columns: 256 rows of the padded row space each
    g.nblk_r = (h->N + 255) / 256;
    const size_t nseg = g.segs.size(), ni = g.items.size(), n = (size_t)g.nslots;
    int rc;
    if ((rc = g.d_segs.alloc(h, nseg)) || (rc = g.d_items.alloc(h, ni)) || (rc = g.d_set_item0.alloc(h, set_item0.size())) ||
        (rc = g.d_set_seg0.alloc(h, set_seg0.size())) || (rc = g.d_slot_seg.alloc(h, slot_seg.size())) || (rc = g.d_slot_e.alloc(h, n)) ||
        (rc = g.d_part.alloc(h, ni * (size_t)h->L)) || (rc = g.d_segm.alloc(h, nseg)) || (rc = g.d_sega.alloc(h, nseg)) ||
        (rc = g.d_acc.alloc(h, 6 * n + 2)) || (rc = g.d_trace.alloc(h, (size_t)g.trace_rows * (n + 1))) ||
        (rc = g.d_qw.alloc(h, (size_t)g.ncol_w * (size_t)g.nwin * 2)) || (rc = g.d_qs.alloc(h, (size_t)g.nblk_r * (nsets + 1) * 2)) ||
        (rc = g.d_cnt.alloc(h, 2)))
        return rc;
    HCHK(hipMemcpyAsync(g.d_segs, g.segs.data(), nseg * sizeof(GvSeg), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(g.d_items, g.items.data(), ni * sizeof(GvItem), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(g.d_set_item0, set_item0.data(), set_item0.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(g.d_set_seg0, set_seg0.data(), set_seg0.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (!slot_seg.empty()) HCHK(hipMemcpyAsync(g.d_slot_seg, slot_seg.data(), slot_seg.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    {   // the range of the stored values: one pass over the panel, an integer maximum (d_cnt[1] is free until the first pass)
        unsigned long long bits = 0ull;
        HCHK(genvar_xmax((const void *)h->pm->tiles.get(), (const double *)h->pm->mean.get(), h->req.storage == 1, (long long)h->N, (long long)h->L,
                         (long long)h->NBLK, (unsigned long long *)(g.d_cnt.get() + 1), h->stream));
        HCHK(hipMemcpyAsync(&bits, g.d_cnt.get() + 1, sizeof bits, hipMemcpyDeviceToHost, h->stream));
        HCHK(hipStreamSynchronize(h->stream));  // (the tables are locals)
        HCHK(hipMemsetAsync(g.d_cnt.get() + 1, 0, sizeof(long long), h->stream));
        double xmax;
        std::memcpy(&xmax, &bits, sizeof xmax);
        g.ex = gv_xexp(xmax);
    }
    g.built = true;
    return NGP_OK;
}

// The chain's variance arrays for the sets and windows it has now: built (zeroed) when either changed, zeroed again on request
// (ngp_set_y).  Nothing to do while the pass is off.
int ensure_diag(ngp_handle *h, bool zero);  // (below)
int ensure_genvar(ngp_handle *h, bool zero) {
    GenVar &g = h->cm.gv;
    if (!g.on || !h->pm || h->records_only || h->sets.empty()) { g.built = false; return NGP_OK; }
    bool same = g.built && g.built_for.size() == 2 * h->sets.size();
    for (size_t s = 0; same && s < h->sets.size(); s++) same = g.built_for[2 * s] == h->sets[s].col0 && g.built_for[2 * s + 1] == h->sets[s].ncol;
    if (!same) return build_genvar(h);
    if (zero) {
        HCHK(hipMemsetAsync(g.d_acc, 0, (size_t)(6 * g.nslots + 2) * sizeof(double), h->stream));
        HCHK(hipMemsetAsync(g.d_cnt, 0, 2 * sizeof(long long), h->stream));
        if (g.trace_rows > 0) HCHK(hipMemsetAsync(g.d_trace, 0, (size_t)g.trace_rows * (size_t)(g.nslots + 1) * sizeof(double), h->stream));
    }
    return NGP_OK;
}

// the same panel, sets and windows: one pass serves both chains
bool same_genvar(const ngp_handle *a, const ngp_handle *b) {
    const GenVar &x = a->cm.gv, &y = b->cm.gv;
    if (a->pm != b->pm || x.built_for != y.built_for || x.segs.size() != y.segs.size()) return false;
    for (size_t i = 0; i < x.segs.size(); i++)
        if (x.segs[i].j0 != y.segs[i].j0 || x.segs[i].j1 != y.segs[i].j1 || x.segs[i].slot != y.segs[i].slot) return false;
    return true;
}

// ONE pass over the training panel for the n chains hs (their sets and windows equal hs[0]'s), on lead's stream: segment scalars and
// scales, the tile pass, the rows' set values, then every chain's V, q, r and sums.  Threshold and trace capacity are each chain's own.
int launch_genvar(ngp_handle *lead, ngp_handle **hs, int n) {
    ngp_handle *h = lead;
    const GenVar &g0 = hs[0]->cm.gv;
    GvLaunch q;
    std::memset(&q, 0, sizeof q);
    for (int i = 0; i < n; i++) {
        ChainMem &c = hs[i]->cm;
        GenVar &g = c.gv;
        q.A.c[i] = GvChain{(const double *)c.d_beta.get(), (const DScal *)c.d_scal.get(), g.d_part.get(), g.d_segm.get(), g.d_sega.get(), g.d_slot_e.get(),
                           g.d_qw.get(), g.d_qs.get(), g.d_acc.get(), g.d_acc.get() + 6 * g.nslots, g.d_trace.get(), g.d_cnt.get()};
        q.thr[i] = g.thr; q.trace_rows[i] = (long long)g.trace_rows;
    }
    q.n = n; q.u8 = lead->req.storage == 1;
    q.tiles = (const void *)lead->pm->tiles.get(); q.mean = (const double *)lead->pm->mean.get();
    q.segs = g0.d_segs.get(); q.items = g0.d_items.get();
    q.slot_seg = g0.d_slot_seg.get(); q.set_seg0 = g0.d_set_seg0.get(); q.set_item0 = g0.d_set_item0.get();
    q.nseg = (int)g0.segs.size(); q.nitems = (int)g0.items.size(); q.nsets = (int)hs[0]->sets.size(); q.nwin = (int)g0.nwin; q.nslots = (int)g0.nslots;
    q.ex = g0.ex; q.ncol_w = (int)g0.ncol_w; q.nblk_r = (int)g0.nblk_r;
    q.N = (long long)lead->N; q.L = (long long)lead->L;
    q.abort_w = lead->cm.d_abort; q.stream = lead->stream;
    const hipError_t e = genvar_launch(q);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("genomic variance pass: ") + hipGetErrorString(e));
    lead->cm.gv.launches += 1;
    lead->cm.gv.served += n;
    return NGP_OK;
}

// one step of a sparse fixed-effect set (ngp_fixed_sparse.h): Yi of every column, the Gauss-Seidel depth by depth, the residual
void launch_fixed_sparse(ngp_handle *h, int f, uint64_t it) {
    const HFix &F = h->mm.fix[(size_t)f];
    const long long nc = (long long)F.ncol;
    const unsigned *ab = (const unsigned *)h->cm.d_abort;
    const DScal *sc = (const DScal *)h->cm.d_scal;
    double *b = h->mm.d_bfix + F.off;
    const long long *xp = F.d_xptr;
    const int *xc = F.d_xcol;
    const double *xv = F.d_xval, *dg = F.d_diagR;
    hipLaunchKernelGGL(k_fixs_yi, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, h->stream, (const double *)h->cm.d_ycorr, nc, (const long long *)F.d_cptr,
                       (const int *)F.d_crow, (const double *)F.d_cval, xp, xc, xv, (const double *)b, F.d_scr.get(), sc, ab);
    for (const HFix::Launch &pl : F.plan) {
        if (pl.wide)
            hipLaunchKernelGGL(k_fixs_gs_wide, dim3((unsigned)((pl.r1 - pl.r0 + 255) / 256)), dim3(256), 0, h->stream, nc, xp, xc, xv, dg, b, F.d_scr.get(),
                               (const int *)F.d_order, pl.r0, pl.r1, sc, f, h->seed, (uint64_t)h->chain, it, ab);
        else
            hipLaunchKernelGGL(k_fixs_gs_fused, dim3(1), dim3(1024), 0, h->stream, nc, xp, xc, xv, dg, b, F.d_scr.get(), (const int *)F.d_order,
                               (const long long *)F.d_dptr, pl.d0, pl.d1, sc, f, h->seed, (uint64_t)h->chain, it, ab);
    }
    hipLaunchKernelGGL(k_fixs_update, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, h->cm.d_ycorr.get(), (long long)h->N, nc,
                       (const long long *)F.d_rptr, (const int *)F.d_rcol, (const double *)F.d_rval, (const double *)F.d_scr.get(), ab);
}

void iteration_pre(ngp_handle *h, int64_t trace_idx, bool resume_mid) {  // everything in front of the sweep
    const uint64_t it = (uint64_t)(h->iter + 1);
    if (!resume_mid) {
    if (const long long m = (long long)h->cm.lb.rows.size()) {  // liability traits: thresholds (C >= 3), then every liability (ycorr_i <- e_i)
        const Liab &lb = h->cm.lb;
        const int C1 = lb.C + 1;
        if (lb.C >= 3 && lb.ts_mode == 1) {  // Cowles' joint move in the place of k_thresholds: proposal and likelihood terms, then the decision
            const int nwg = (int)((m + NGP_THR_WG - 1) / NGP_THR_WG);
            hipLaunchKernelGGL(k_threshold_terms, dim3((unsigned)nwg), dim3(NGP_THR_WG), 0, h->stream, (const long long *)lb.d_rows.get(), (const int *)lb.d_cls.get(),
                               (const double *)lb.d_liab.get(), m, lb.C, (const double *)h->cm.d_ycorr.get(), (const double *)h->cm.d_rs, (const DScal *)h->cm.d_scal,
                               (const double *)lb.d_thr.get(), (const ThrStep *)lb.d_ts.get(), lb.d_tg.get(), lb.d_tpart.get(), h->seed, (uint64_t)h->chain, it,
                               h->hm.d_tn_fall.get(), (const unsigned *)h->cm.d_abort);
            hipLaunchKernelGGL(k_threshold_decide, dim3(1), dim3(64), 0, h->stream, lb.C, lb.d_thr.get(), lb.d_thr.get() + C1, lb.d_thr.get() + 2 * C1,
                               (const double *)lb.d_tg.get(), (const double *)lb.d_tpart.get(), nwg, lb.d_ts.get(), (int)is_kept(h, h->iter + 1),
                               (int)(lb.ts_adapt && h->iter + 1 <= h->burnIn), h->seed, (uint64_t)h->chain, it, (const unsigned *)h->cm.d_abort);
        } else if (lb.C >= 3)
            hipLaunchKernelGGL(k_thresholds, dim3(1), dim3(1024), 0, h->stream, (const int *)lb.d_cls.get(), (const double *)lb.d_liab.get(), m, lb.C, lb.d_thr.get(),
                               lb.d_thr.get() + C1, lb.d_thr.get() + 2 * C1, (int)is_kept(h, h->iter + 1), h->seed, (uint64_t)h->chain, it, (const unsigned *)h->cm.d_abort);
        hipLaunchKernelGGL(k_liability_augment, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, (const long long *)lb.d_rows.get(), m, h->cm.d_ycorr.get(),
                           lb.d_liab.get(), (const double *)lb.d_lo.get(), (const double *)lb.d_hi.get(), (const int *)lb.d_cls.get(), (const double *)lb.d_thr.get(),
                           (const double *)h->cm.d_rs, (const DScal *)h->cm.d_scal, h->seed, (uint64_t)h->chain, it, h->hm.d_tn_fall.get(), (const unsigned *)h->cm.d_abort);
    }
    if (const long long m = (long long)h->cm.ho_rows.size())  // held-out records: their phenotypes are redrawn first (ycorr_i <- e_i)
        hipLaunchKernelGGL(k_holdout_augment, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, (const long long *)h->cm.d_ho_rows, m, h->cm.d_ycorr.get(),
                           h->cm.d_yaug.get(), (const double *)h->cm.d_rs, (const DScal *)h->cm.d_scal, h->seed, (uint64_t)h->chain, it, (const unsigned *)h->cm.d_abort);
    hipLaunchKernelGGL(k_head, dim3(1), dim3(1024), 0, h->stream, h->cm.d_ycorr, (long long)h->L, (long long)h->N, h->cm.d_scal, h->e_df,
                       h->e_scale, h->intercept, h->fix_varE > 0.0 ? 0 : 1, h->seed, (uint64_t)h->chain, it, h->hm.d_tr_varE, h->hm.d_tr_b, (long long)trace_idx, h->cm.d_abort, h->pm->mpm_max,
                       (const double *)h->cm.d_rs, h->sum_w);
    for (size_t f = 0; f < h->mm.fix.size(); f++)  // the other fixed-effect sets, in the order they were added (src/samplers.jl:39-41)
        if (h->mm.fix[f].sparse) launch_fixed_sparse(h, (int)f, it);
        else hipLaunchKernelGGL(k_fixed, dim3(1), dim3(1024), 0, h->stream, h->cm.d_ycorr, (long long)h->N, h->mm.fix[f].d_X, (int)h->mm.fix[f].ncol, h->mm.fix[f].d_xpx0,
                           h->mm.fix[f].d_xpxR, h->mm.fix[f].d_lhs0, h->mm.fix[f].d_rhs0, h->mm.d_bfix + h->mm.fix[f].off, h->cm.d_scal, (int)f, h->seed,
                           (uint64_t)h->chain, it, h->cm.d_abort);
    for (size_t r = 0; r < h->mm.rnd.size(); r++)  // the random-effect sets, in the order they were added (src/samplers.jl:43-46)
        launch_random(h, (int)r, it);
    }
    if (h->records_only) return;  // no marker set: no coefficients, no sweep
    hipLaunchKernelGGL(k_prep, dim3((unsigned)(h->Ppad / 256 + 1)), dim3(256), 0, h->stream, (long long)h->Ppad, h->cm.d_setof, h->cm.d_loc,
                       h->cm.d_vbidx, h->cm.d_sets, h->cm.d_scal, h->mm.d_varBeta, h->pm->mpm, h->cm.d_lhs0, h->cm.d_rhs0, h->cm.d_beta, h->cm.d_c, h->cm.d_w,
                       h->cm.d_q, h->cm.d_T, h->cm.d_chi, -1, h->seed, (uint64_t)h->chain, it, (long long)h->h_regs.size(), h->mm.d_regs, h->mm.d_regchi, h->mm.d_rcls,
                       h->cm.d_ccnt, (long long)(h->plan.mode == 1 ? h->cm.ccnt_words : 0), h->cm.d_abort, h->mm.d_tup, h->mm.d_tupc, h->mm.d_tupg, (const DRc *)h->mm.d_rctab.get());
    launch_tinv(h);
}

// predict: this chain launches its own prediction pass in a kept iteration (false: the caller serves several chains with one launch)
// genvar: the same for the genomic-variance pass
int iteration_post(ngp_handle *h, int64_t trace_idx, bool predict = true, bool genvar = true) {  // variance / pi draws, traces and posterior sums; advances h->iter
    const uint64_t it = (uint64_t)(h->iter + 1);
    if (!h->records_only) launch_variance(h, -1, it);
    h->iter += 1;
    const bool do_trace = h->mm.d_trace_loci && trace_idx < h->mm.trace_ext_cap, do_accum = is_kept(h, h->iter);
    if (do_trace || do_accum) {
        long long n = 16;
        if (do_trace) n = std::max<long long>(n, std::max<long long>(std::max<long long>(h->mm.ntl, h->mm.ntvb), (long long)h->sets.size()));
        if (do_accum) n = std::max<long long>(n, std::max<long long>(h->P, h->nvb));
        hipLaunchKernelGGL(k_post, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (int)do_accum, (long long)h->P, (long long)h->nvb,
                           (int)h->sets.size(), h->cm.d_beta, h->cm.d_delta, h->mm.d_varBeta, h->cm.d_sum_beta, h->cm.d_sum_beta2, h->cm.d_sum_delta,
                           h->mm.d_sum_varBeta, h->cm.d_sets, h->cm.d_scal, (int)do_trace, (long long)h->mm.ntl, (const long long *)h->mm.d_trace_loci.get(),
                           (long long)h->mm.ntvb, h->mm.d_tr_beta, h->mm.d_tr_vb, h->mm.d_tr_pi, (long long)trace_idx, h->cm.d_abort);
    }
    if (do_accum) {
        if (h->mm.nfixcol > 0)
            hipLaunchKernelGGL(k_accum_fixed, dim3((unsigned)((h->mm.nfixcol + 255) / 256)), dim3(256), 0, h->stream, (long long)h->mm.nfixcol, h->mm.d_bfix,
                               h->mm.d_sum_bfix, h->cm.d_abort);
        for (auto &R : h->mm.rnd) {  // random-effect sets: u and varU (src/samplers.jl:60-75)
            const long long qk = (long long)R.q * R.tk, kk = (long long)R.tk * R.tk;
            hipLaunchKernelGGL(k_accum_fixed, dim3((unsigned)((qk + 255) / 256)), dim3(256), 0, h->stream, qk, R.d_u, R.d_sum_u, h->cm.d_abort);
            hipLaunchKernelGGL(k_accum_fixed, dim3(1), dim3(64), 0, h->stream, kk, R.d_vu, R.d_vu + kk, h->cm.d_abort);
        }
        for (auto &V : h->mm.lv)  // BayesLV sets: c and varZeta (src/samplers.jl:89-92)
            hipLaunchKernelGGL(k_accum_fixed, dim3(1), dim3(64), 0, h->stream, (long long)NGP_LV_SUM, V.d_st, V.d_st + NGP_LV_SUM, h->cm.d_abort);
        for (auto &Rc : h->mm.rc)  // BayesRCpi sets: the annotation category of every locus (src/samplers.jl:85-87)
            hipLaunchKernelGGL(k_rc_accum, dim3((unsigned)((Rc.n + 255) / 256)), dim3(256), 0, h->stream, (const DSet *)h->cm.d_sets, Rc.set, Rc.dev(),
                               (const unsigned *)h->cm.d_abort);
        if (const long long m = (long long)h->cm.ho_rows.size())  // held-out records: the fitted value of this draw
            hipLaunchKernelGGL(k_holdout_accum, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, (const long long *)h->cm.d_ho_rows, m,
                               (const double *)h->cm.d_ycorr, (const double *)h->cm.d_yaug, (const double *)h->cm.d_rs, h->cm.d_sum_fit.get(), h->cm.d_sum_fit2.get(),
                               h->cm.d_n_fit.get(), (const unsigned *)h->cm.d_abort);
        if (h->cm.lb.d_sum_prob) {  // ... and their class probabilities under the thresholds of this draw
            const Liab &lb = h->cm.lb;
            const long long m = (long long)h->cm.ho_rows.size();
            hipLaunchKernelGGL(k_holdout_prob, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, (const long long *)h->cm.d_ho_rows, m, lb.C,
                               (const double *)h->cm.d_ycorr, (const double *)h->cm.d_yaug, (const double *)h->cm.d_rs, (const DScal *)h->cm.d_scal,
                               (const double *)lb.d_thr.get(), lb.d_sum_prob.get(), (const unsigned *)h->cm.d_abort);
        }
        if (predict && predicts(h)) launch_predict(h, &h, 1);  // g = X_new beta of this draw, behind the posterior sums
        if (genvar && gv_active(h))                            // var(X beta) of this draw per window, set and in all
            if (int e = launch_genvar(h, &h, 1)) return e;
        if (h->cm.dg.on && h->cm.dg.D > 0) launch_diag(h);     // the lag-window autocovariance of every monitored scalar takes this draw
        if (h->smp) return sample_enqueue(h);  // the kept sample goes to the file without stopping the chain (src/samplers.jl:56-104)
    }
    return NGP_OK;
}

// resume_mid: the head of this iteration (varE, intercept, fixed-effect sets) has run already -- its sweep ended at the census
// with nothing changed and is launched again, k_prep first (it redraws the same keyed numbers and clears the hand-off counters)
int one_iteration(ngp_handle *h, int64_t trace_idx, hipEvent_t *evs, bool resume_mid = false) {
    iteration_pre(h, trace_idx, resume_mid);
    if (!h->records_only) launch_sweep(h, 0, h->NBLK, evs);
    return iteration_post(h, trace_idx);
}

// niter iterations from the handle's current state under `lease`, the launch queue bounded to 16 iterations; a launch that ends at
// its census (grid not co-resident beside another chain's, nothing changed) is run again once the device is this call's alone
int run_iterations(ngp_handle *h, int64_t niter, CuLease &lease, hipEvent_t *evs_first) {
    int rc;
    const int64_t iter0 = h->iter;
    bool resume_mid = false;
    int64_t n = 0;
    while (n < niter) {
        if ((rc = one_iteration(h, n, (n == 0) ? evs_first : nullptr, resume_mid))) return rc;
        resume_mid = false;
        ++n;
        if ((n & 15) == 0 || n == niter) {  // bound the launch queue
            HCHK(hipStreamSynchronize(h->stream));
            int64_t itf = 0;
            rc = check_abort(h, &itf);
            if (rc == NGP_RETRY_CENSUS) {
                // kernels behind the failing launch returned at once (abort word): the chain stands at iteration itf, head done
                h->exclusive = true; h->census_retries += 1;
                lease.make_exclusive();
                if (predicts(h))  // the prediction passes behind the failing launch returned at once: they are launched again
                    for (int64_t r = itf; r <= h->iter; r++)
                        if (is_kept(h, r)) { h->cm.pred_launches -= 1; h->cm.pred_served -= 1; }
                if (gv_active(h))  // ... and so are the variance passes
                    for (int64_t r = itf; r <= h->iter; r++)
                        if (is_kept(h, r)) { h->cm.gv.launches -= 1; h->cm.gv.served -= 1; }
                if (h->cm.dg.on && h->cm.dg.D > 0)  // ... and the diagnostics updates: their draw index goes back with the iteration
                    for (int64_t r = itf; r <= h->iter; r++)
                        if (is_kept(h, r)) { h->cm.dg.n -= 1; h->cm.dg.launches -= 1; }
                h->iter = itf - 1;
                n = h->iter - iter0;
                resume_mid = true;
                continue;
            }
            if (rc) return rc;
        }
    }
    return NGP_OK;
}

// class probabilities / their posterior sums of a BayesR set (either may be null); also clears the class counters
int set_class_state_dev(ngp_handle *h, int si, int K, const double *pi, const double *sum_pi) {
    DevArray<double> d;
    int rc;
    if ((rc = d.alloc(h, (size_t)2 * NGP_RMAX))) return rc;
    if (pi) HCHK(hipMemcpyAsync(d, pi, (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (sum_pi) HCHK(hipMemcpyAsync(d + NGP_RMAX, sum_pi, (size_t)K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_set_class_state, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, si, K, pi ? d.get() : nullptr, sum_pi ? d + NGP_RMAX : nullptr);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("class state: ") + hipGetErrorString(e));
    return NGP_OK;
}

// ---- liability traits (ngp_liability.h) ----
// the counter of truncated-normal draws that ran out of rounds: one word of the handle, allocated (zeroed) on first use
int ensure_tn_fall(ngp_handle *h) {
    return h->hm.d_tn_fall ? NGP_OK : h->hm.d_tn_fall.alloc(h, 1);
}
uint64_t liab_digest(const Liab &lb) {  // FNV-1a over the rows, C and the classes or bounds
    uint64_t d = 1469598103934665603ull;
    auto eat = [&d](const void *p, size_t n) { for (size_t i = 0; i < n; i++) { d ^= ((const unsigned char *)p)[i]; d *= 1099511628211ull; } };
    eat(lb.rows.data(), lb.rows.size() * sizeof(long long));
    eat(&lb.C, sizeof lb.C);
    eat(lb.cls.data(), lb.cls.size() * sizeof(int));
    eat(lb.lo.data(), lb.lo.size() * 8); eat(lb.hi.data(), lb.hi.size() * 8);
    return d;
}
// ... as the snapshot signature carries it: the word ts_mode + 2 (class probabilities on) is folded in where it is not 0, so a chain
// under Albert-Chib without class probabilities keeps the digest every earlier snapshot has
uint64_t liab_sig_digest(uint64_t digest, int ts_mode, bool prob) {
    const uint32_t w = (uint32_t)ts_mode + (prob ? 2u : 0u);
    if (w == 0) return digest;
    uint64_t d = digest;
    for (int i = 0; i < 4; i++) { d ^= (unsigned char)((w >> (8 * i)) & 0xff); d *= 1099511628211ull; }
    return d;
}
// Start values (ngp_set_y; DESIGN.md section 2, "Liability traits").  Classes: t_c = ppnd16(F_c) - ppnd16(F_1) with F_c the cumulative
// class frequency over the augmented rows (ppnd16 on the device: the draw layer's own), the liability the midpoint of an inner
// interval, t_1 - 0.5 in class 1, t_{C-1} + 0.5 in class C.  Bounds: the finite bound where only one is, else the midpoint.  y_out: y
// with the liability on every augmented row (classes: 0 elsewhere -- y is not read); left empty for a chain without liabilities.
int start_liabilities(ngp_handle *h, const double *y, std::vector<double> &y_out) {
    Liab &lb = h->cm.lb;
    if (!lb.on()) return NGP_OK;
    int rc;
    const size_t m = lb.rows.size(), C1 = (size_t)lb.C + 1;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> l0(m), thr(3 * C1, 0.0);
    if (lb.C >= 2) {
        const int C = lb.C;
        std::vector<long long> cnt((size_t)C + 1, 0);
        for (int c : lb.cls) cnt[(size_t)c] += 1;
        std::vector<double> F((size_t)C - 1), q((size_t)C - 1);
        long long cum = 0;
        for (int c = 1; c < C; c++) { cum += cnt[(size_t)c]; F[(size_t)c - 1] = (double)cum / (double)m; }
        DevArray<double> di, dq;
        if ((rc = di.alloc(h, F.size())) || (rc = dq.alloc(h, F.size()))) return rc;
        HCHK(hipMemcpyAsync(di, F.data(), F.size() * 8, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_eval_math, dim3(1), dim3(64), 0, h->stream, 1, (const double *)di.get(), (long long)F.size(), dq.get());
        HCHK(hipMemcpyAsync(q.data(), dq, q.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HCHK(hipStreamSynchronize(h->stream));
        thr[0] = -inf; thr[(size_t)C] = inf;
        for (int c = 1; c < C; c++) thr[(size_t)c] = q[(size_t)c - 1] - q[0];
        for (size_t k = 0; k < m; k++) {
            const int c = lb.cls[k];
            l0[k] = c == 1 ? thr[1] - 0.5 : c == C ? thr[(size_t)C - 1] + 0.5 : (thr[(size_t)c - 1] + thr[(size_t)c]) / 2.0;
        }
        y_out.assign((size_t)h->N, 0.0);
        HCHK(hipMemcpy(lb.d_thr, thr.data(), thr.size() * 8, hipMemcpyHostToDevice));
        if (lb.ts_mode == 1) {  // a fresh chain: the proposal SD it starts with, nothing proposed yet
            const ThrStep t0{lb.ts_sigma0, 0, 0};
            HCHK(hipMemcpy(lb.d_ts, &t0, sizeof t0, hipMemcpyHostToDevice));
        }
        if (lb.d_sum_prob) HCHK(hipMemset(lb.d_sum_prob, 0, (size_t)C * h->cm.ho_rows.size() * 8));
    } else {
        for (size_t k = 0; k < m; k++) {
            const bool fl = std::isfinite(lb.lo[k]), fh = std::isfinite(lb.hi[k]);
            l0[k] = (fl && fh) ? (lb.lo[k] + lb.hi[k]) / 2.0 : fl ? lb.lo[k] : lb.hi[k];
        }
        y_out.assign(y, y + h->N);
    }
    for (size_t k = 0; k < m; k++) y_out[(size_t)lb.rows[k]] = l0[k];
    HCHK(hipMemcpy(lb.d_liab, l0.data(), m * 8, hipMemcpyHostToDevice));
    return NGP_OK;
}

// ---- the chain's state as segments (ngp_state.h: the segment ids, the three layouts, the formats) ----
// every segment of h's chain.  No device access: the staged words (st.ds, st.sc) are filled by stage()
void describe(ngp_handle *h, ChainState &st) {
    const size_t P8 = (size_t)h->P * 8, vb8 = (size_t)h->nvb * 8, fx8 = (size_t)h->mm.nfixcol * 8;
    st.ds.resize(h->sets.size());
    st.nfix = h->mm.nfixcol; st.chain64 = h->chain;
    st.host(SEG_ITER, 0, &h->iter, 8); st.host(SEG_SEED, 0, &h->seed, 8); st.host(SEG_CHAIN, 0, &st.chain64, 8); st.host(SEG_NFIX, 0, &st.nfix, 8);
    st.host(SEG_VARE, 0, &st.sc.varE, 8); st.host(SEG_B, 0, &st.sc.b, 8);
    st.host(SEG_SUM_VARE, 0, &st.sc.sum_varE, 8); st.host(SEG_SUM_B, 0, &st.sc.sum_b, 8);
    st.host(SEG_NKEPT, 0, &st.sc.nKept, 8); st.host(SEG_NKEPT_F64, 0, &st.nkept_f64, 8);
    st.dev(SEG_YCORR, 0, h->cm.d_ycorr, (size_t)h->N * 8); st.dev(SEG_BETA, 0, h->cm.d_beta, P8); st.dev(SEG_DELTA, 0, h->cm.d_delta, (size_t)h->P);
    st.dev(SEG_SUM_BETA, 0, h->cm.d_sum_beta, P8); st.dev(SEG_SUM_BETA2, 0, h->cm.d_sum_beta2, P8); st.dev(SEG_SUM_DELTA, 0, h->cm.d_sum_delta, P8);
    st.dev(SEG_VARBETA, 0, h->mm.d_varBeta, vb8); st.dev(SEG_SUM_VARBETA, 0, h->mm.d_sum_varBeta, vb8);
    st.dev(SEG_FIX, 0, h->mm.d_bfix, fx8); st.dev(SEG_SUM_FIX, 0, h->mm.d_sum_bfix, fx8);
    for (int s = 0; s < (int)h->sets.size(); s++) {
        DSet &d = st.ds[(size_t)s];
        const size_t K8 = (size_t)h->sets[(size_t)s].K * 8;
        st.host(SEG_FINE, s, &h->sets[(size_t)s].fine_calls, 8);
        st.host(SEG_PI, s, &d.piHat0, 16); st.host(SEG_SUM_PI, s, &d.sum_pi0, 16);  // (piHat0 | piHat1 and sum_pi0 | sum_pi1 are neighbours)
        if (K8) { st.host(SEG_CLS, s, d.pic, K8); st.host(SEG_SUM_CLS, s, d.sum_pic, K8); }
    }
    for (int r = 0; r < (int)h->mm.rnd.size(); r++) {
        HRand &R = h->mm.rnd[(size_t)r];
        const size_t qk8 = (size_t)R.q * (size_t)R.tk * 8, kk = (size_t)R.tk * (size_t)R.tk;  // (a tuple set: u is q x k, varU k x k)
        st.dev(SEG_U, r, R.d_u, qk8); st.dev(SEG_SUM_U, r, R.d_sum_u, qk8);
        st.dev(SEG_VARU, r, R.d_vu, kk * 8); st.dev(SEG_SUM_VARU, r, R.d_vu + kk, kk * 8); st.dev(SEG_VU, r, R.d_vu, 2 * kk * 8);
        st.host(SEG_RFINE, r, &R.fine_calls, 8);
    }
    for (int v = 0; v < (int)h->mm.lv.size(); v++) {
        HLv &V = h->mm.lv[(size_t)v];
        st.dev(SEG_LV, v, V.d_st, NGP_LV_SUM * 8); st.dev(SEG_SUM_LV, v, V.d_st + NGP_LV_SUM, NGP_LV_SUM * 8);
        st.dev(SEG_LV_ALL, v, V.d_st, NGP_LV_WORDS * 8); st.dev(SEG_ZETA, v, V.d_zeta, (size_t)V.n * 8);
    }
    for (int r = 0; r < (int)h->mm.rc.size(); r++) {  // (pi, its sums and the A variances of such a set: SEG_CLS, SEG_SUM_CLS, SEG_VARBETA)
        HRc &Rc = h->mm.rc[(size_t)r];
        const size_t an8 = (size_t)Rc.A * (size_t)Rc.n * 8;
        st.dev(SEG_RC_PROB, r, Rc.d_prob, an8); st.dev(SEG_RC_CAT, r, Rc.d_cat, (size_t)Rc.n); st.dev(SEG_SUM_RC, r, Rc.d_sum, an8);
    }
    if (!h->cm.ho_rows.empty()) {  // held-out records: only a chain with a mask has these segments
        const size_t N8 = (size_t)h->N * 8;
        st.dev(SEG_YAUG, 0, h->cm.d_yaug, h->cm.ho_rows.size() * 8);
        st.dev(SEG_SUM_FIT, 0, h->cm.d_sum_fit, N8); st.dev(SEG_SUM_FIT2, 0, h->cm.d_sum_fit2, N8); st.dev(SEG_N_FIT, 0, h->cm.d_n_fit, N8);
    }
    if (h->cm.lb.on()) {  // liability traits: only a chain that has them; the thresholds t_1 .. t_{C-1} and their sums only with classes
        const Liab &lb = h->cm.lb;
        st.dev(SEG_LIAB, 0, lb.d_liab, lb.rows.size() * 8);
        if (lb.C >= 2) {
            const size_t C1 = (size_t)lb.C + 1;
            st.dev(SEG_THR, 0, lb.d_thr + 1, lb.thr_bytes());
            st.dev(SEG_SUM_THR, 0, lb.d_thr + C1 + 1, lb.thr_bytes()); st.dev(SEG_SUM_THR2, 0, lb.d_thr + 2 * C1 + 1, lb.thr_bytes());
            if (lb.C >= 3) st.dev(SEG_THR_SMP, 0, lb.d_thr + 2, (size_t)(lb.C - 2) * 8);  // the drawn thresholds: what a sample record carries
            if (lb.ts_mode == 1) st.dev(SEG_THR_STEP, 0, lb.d_ts, sizeof(ThrStep));        // Cowles' step: sigma | tries | accepted
            if (lb.d_sum_prob) st.dev(SEG_SUM_PROB, 0, lb.d_sum_prob, (size_t)lb.C * h->cm.ho_rows.size() * 8);
        }
    }
}
static_assert(offsetof(DSet, piHat1) == offsetof(DSet, piHat0) + 8 && offsetof(DSet, sum_pi1) == offsetof(DSet, sum_pi0) + 8, "SEG_PI / SEG_SUM_PI");

// the words of DSet and DScal into their staging (one copy each)
int stage(ngp_handle *h, ChainState &st) {
    HCHK(hipStreamSynchronize(h->stream));
    if (!st.ds.empty()) HCHK(hipMemcpy(st.ds.data(), h->cm.d_sets, st.ds.size() * sizeof(DSet), hipMemcpyDeviceToHost));
    HCHK(hipMemcpy(&st.sc, h->cm.d_scal, sizeof(DScal), hipMemcpyDeviceToHost));
    st.nkept_f64 = (double)st.sc.nKept;
    return NGP_OK;
}

// ... and back, through the setters: the values (piHat, class probabilities, varE, b), the posterior sums, or both.  k_set_pi
// recomputes logPi and clears nloci, k_set_class_state recomputes logpic and clears ncls (also for the sums alone), iVarE = 1 / varE.
int commit(ngp_handle *h, ChainState &st, bool values, bool sums) {
    int rc;
    for (int s = 0; s < (int)st.ds.size(); s++) {
        DSet &d = st.ds[(size_t)s];
        if (values) hipLaunchKernelGGL(k_set_pi, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, s, d.piHat0, d.piHat1);
        if (sums) hipLaunchKernelGGL(k_set_sum_pi, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, s, d.sum_pi0, d.sum_pi1);
        if (h->sets[(size_t)s].K > 0 && (rc = set_class_state_dev(h, s, h->sets[(size_t)s].K, values ? d.pic : nullptr, sums ? d.sum_pic : nullptr))) return rc;
    }
    DScal sc;  // (the other words -- db, the fixed-point scales -- stay as they are on the device)
    HCHK(hipMemcpy(&sc, h->cm.d_scal, sizeof(DScal), hipMemcpyDeviceToHost));
    if (values) { sc.varE = st.sc.varE; sc.iVarE = 1.0 / sc.varE; sc.b = st.sc.b; }
    if (sums) { sc.sum_varE = st.sc.sum_varE; sc.sum_b = st.sc.sum_b; sc.nKept = st.sc.nKept; }
    HCHK(hipMemcpy(h->cm.d_scal, &sc, sizeof(DScal), hipMemcpyHostToDevice));
    HCHK(hipStreamSynchronize(h->stream));
    return NGP_OK;
}

// doubles of the packed posterior (ngp_posterior_len)
int64_t posterior_words(ngp_handle *h) {
    ChainState st;
    describe(h, st);
    return (int64_t)(place(st, posterior_layout).bytes / 8);
}

// ---- convergence diagnostics (ngp_diag.h; DESIGN.md section 2, "Convergence diagnostics") ----
// The gather table and the state for the model the chain has now: D and the order come from diag_layout; a word staged on the host
// (DScal, DSet) is read where it lives on the device.  Allocated (zeroed) when D changed -- an error once draws are held --, zeroed
// again on request (ngp_set_y).  Nothing to do while the diagnostics are off.
int ensure_diag(ngp_handle *h, bool zero) {
    Diag &g = h->cm.dg;
    if (!g.on) return NGP_OK;
    ChainState st;
    describe(h, st);
    const Plan pl = place(st, diag_layout);
    const int64_t D = (int64_t)(pl.bytes / 8), Dp = (D + 1) / 2 * 2;
    std::vector<DiagSeg> segs;
    int64_t maxw = 0;
    for (auto &a : pl.at) {
        if (a.s->bytes == 0) continue;
        const char *src = (const char *)a.s->p;
        if (a.s->host) {
            const char *sc0 = (const char *)&st.sc, *ds0 = (const char *)st.ds.data();
            if (src >= sc0 && src < sc0 + sizeof(DScal)) src = (const char *)h->cm.d_scal.get() + (src - sc0);
            else if (!st.ds.empty() && src >= ds0 && src < ds0 + st.ds.size() * sizeof(DSet)) src = (const char *)h->cm.d_sets.get() + (src - ds0);
            else return fail(h, NGP_ERR_STATE, "internal: a monitored word lives on the host only");
        }
        segs.push_back(DiagSeg{(const double *)src, (long long)(a.off / 8), (long long)(a.s->bytes / 8)});
        maxw = std::max<int64_t>(maxw, (int64_t)(a.s->bytes / 8));
    }
    const size_t rows = (size_t)DiagRows::rows(g.L);
    if (zero) { g.n = 0; g.fixed = false; }
    if (D != g.D) {
        REQUIRE(!g.fixed, NGP_ERR_STATE, "the model changed while the convergence diagnostics hold draws (ngp_enable_diagnostics again)");
        g.D = 0; g.Dp = 0; g.segs.clear();
        int rc;
        if ((rc = g.d_st.alloc(h, rows * (size_t)Dp)) || (rc = g.d_x.alloc(h, (size_t)Dp))) {
            g.on = false; g.d_st.reset(); g.d_x.reset(); g.d_segs.reset(); g.seg_cap = 0;  // (the handle runs on without them)
            (void)hipGetLastError();  // (... and its next run does not find the failed hipMalloc in the runtime's error word)
            return rc;
        }
        g.D = D; g.Dp = Dp; g.n = 0;
    } else if (zero && D > 0) {
        HCHK(hipMemsetAsync(g.d_st, 0, rows * (size_t)Dp * sizeof(double), h->stream));
    }
    bool same = segs.size() == g.segs.size();
    for (size_t i = 0; same && i < segs.size(); i++) same = segs[i].src == g.segs[i].src && segs[i].off == g.segs[i].off && segs[i].words == g.segs[i].words;
    if (!same) {
        if (segs.size() > g.seg_cap) {  // (a model of the same D in more runs: the table grows)
            int rc;
            HCHK(hipStreamSynchronize(h->stream));
            if ((rc = g.d_segs.alloc(h, segs.size()))) { g.seg_cap = 0; g.segs.clear(); return rc; }
            g.seg_cap = segs.size();
        }
        g.segs = segs; g.maxw = maxw;
        HCHK(hipMemcpyAsync(g.d_segs, g.segs.data(), g.segs.size() * sizeof(DiagSeg), hipMemcpyHostToDevice, h->stream));
        HCHK(hipStreamSynchronize(h->stream));
    }
    return NGP_OK;
}

// the kept draw of the iteration just enqueued on h->stream: gather theta, then the update for draw index n
void launch_diag(ngp_handle *h) {
    Diag &g = h->cm.dg;
    const unsigned *ab = (const unsigned *)h->cm.d_abort;
    hipLaunchKernelGGL(k_diag_gather, dim3((unsigned)((g.maxw + 255) / 256), (unsigned)g.segs.size()), dim3(256), 0, h->stream, (const DiagSeg *)g.d_segs.get(),
                       g.d_x.get(), ab);
    const long long np = (long long)(g.Dp / 2);
    hipLaunchKernelGGL(k_diag_update, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, (const double2 *)g.d_x.get(), (double2 *)g.d_st.get(), np, g.L,
                       (long long)g.n, (long long)g.split, ab);
    g.n += 1; g.launches += 1; g.fixed = true;
}

// ---- sample stream (ngp_set_sample_file) ----
void sample_writer_loop(SampleStream *S) {
    (void)hipSetDevice(S->device);
    for (;;) {
        int slot;
        {
            std::unique_lock<std::mutex> lk(S->mu);
            S->cv.wait(lk, [&] { return S->stop || !S->queue.empty(); });
            if (S->queue.empty()) return;  // stop, and nothing left
            slot = S->queue.front();
        }
        const bool ok = hipEventSynchronize(S->ev_copied[slot]) == hipSuccess;
        const long long it = *(const long long *)S->h_slot[slot].get();
        bool wrote = false, bad = !ok;
        if (ok && it >= 0) { wrote = true; bad = std::fwrite(S->h_slot[slot], 1, S->rec_bytes, S->f.get()) != S->rec_bytes; }
        {
            std::lock_guard<std::mutex> lk(S->mu);
            S->queue.pop_front();
            S->busy[slot] = false;
            if (bad) S->io_error = true;
            if (wrote && !bad) S->nwritten++; else if (!wrote) S->ndropped++;
        }
        S->cv.notify_all();
    }
}
SampleStream::~SampleStream() {  // (the members -- ring slots, file -- are freed after this body: once the writer has stopped)
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv.notify_all();
    if (writer.joinable()) writer.join();
    for (int i = 0; i < NSLOT; i++) {
        if (ev_packed[i]) (void)hipEventDestroy(ev_packed[i]);
        if (ev_copied[i]) (void)hipEventDestroy(ev_copied[i]);
    }
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
}
// the kept sample of the iteration just enqueued on h->stream goes into the next ring slot, from there to the host on the copy stream
int sample_enqueue(ngp_handle *h) {
    SampleStream *S = h->smp.get();
    ChainState st;
    describe(h, st);
    const Plan pl = place(st, sample_layout, 8);  // (delta's bytes end the record: padded to whole words)
    if (!S->header_written) {  // the model is final now: sizes and the file header
        S->rec_bytes = pl.bytes;
        for (int i = 0; i < SampleStream::NSLOT; i++) {
            if (S->d_slot[i].alloc_raw(S->rec_bytes) != hipSuccess || S->h_slot[i].alloc_raw(S->rec_bytes) != hipSuccess)
                return fail(h, NGP_ERR_NOMEM, "sample ring");
            HCHK(hipMemsetAsync(S->d_slot[i], 0, S->rec_bytes, h->stream));  // (the record's pad bytes: the file does not depend on what the allocator hands out)
        }
        const int64_t hd[6] = {h->P, h->nvb, (int64_t)h->sets.size(), h->mm.nfixcol, h->nclass_total, (int64_t)S->rec_bytes};
        // (the header, by magic: ngp_state.h)
        const bool has_thr = h->cm.lb.C >= 3;               // (05 holds the parts of 04, also when empty)
        const bool has_rc = !h->mm.rc.empty() || has_thr;
        const bool has_lv = !h->mm.lv.empty() || has_rc;  // (04 holds the parts of 03, also when empty)
        bool ok = std::fwrite(has_thr ? "NGPSMP05" : has_rc ? "NGPSMP04" : has_lv ? "NGPSMP03" : h->mm.rnd.empty() ? "NGPSMP01" : "NGPSMP02", 1, 8, S->f.get()) == 8 && std::fwrite(hd, sizeof(hd), 1, S->f.get()) == 1;
        for (auto &hs : h->sets) { const int64_t sg[6] = {hs.method, hs.K, hs.col0, hs.ncol, (int64_t)hs.vb0.size(), hs.tk}; ok = ok && std::fwrite(sg, sizeof(sg), 1, S->f.get()) == 1; }
        if (!h->mm.rnd.empty() || has_lv) {
            const int64_t nr = (int64_t)h->mm.rnd.size();
            ok = ok && std::fwrite(&nr, 8, 1, S->f.get()) == 1;
            for (auto &R : h->mm.rnd) { const int64_t qw = rand_q_word(R); ok = ok && std::fwrite(&qw, 8, 1, S->f.get()) == 1; }
        }
        if (has_lv) {
            const int64_t nl = (int64_t)h->mm.lv.size();
            ok = ok && std::fwrite(&nl, 8, 1, S->f.get()) == 1;
            for (auto &V : h->mm.lv) { const int64_t lg[2] = {V.set, V.ncov}; ok = ok && std::fwrite(lg, sizeof(lg), 1, S->f.get()) == 1; }
        }
        if (has_rc) {
            const int64_t nrc = (int64_t)h->mm.rc.size();
            ok = ok && std::fwrite(&nrc, 8, 1, S->f.get()) == 1;
            for (auto &Rc : h->mm.rc) { const int64_t rg[3] = {Rc.set, Rc.A, Rc.Kc}; ok = ok && std::fwrite(rg, sizeof(rg), 1, S->f.get()) == 1; }
        }
        if (has_thr) {
            const int64_t nthr = h->cm.lb.C - 2;
            ok = ok && std::fwrite(&nthr, 8, 1, S->f.get()) == 1;
        }
        if (!ok) return fail(h, NGP_ERR_ARG, "cannot write the sample file header: " + S->path);
        S->header_written = true;
    } else if (S->rec_bytes != pl.bytes) {
        return fail(h, NGP_ERR_STATE, "the model changed while a sample file is open (ngp_set_sample_file again)");
    }
    const int slot = (int)(S->nenq % SampleStream::NSLOT);
    {
        std::unique_lock<std::mutex> lk(S->mu);
        S->cv.wait(lk, [&] { return !S->busy[slot]; });  // only when the writer is NSLOT samples behind
        if (S->io_error) return fail(h, NGP_ERR_ARG, "writing the sample file failed: " + S->path);
        S->busy[slot] = true;
    }
    // k_sample_pack writes the scalars, b_fixed, beta, varBeta, pi, the class probabilities and delta; it places beta behind b_fixed
    // and a gap, delta behind the class probabilities and a gap: the gaps are read off the plan, and what lies in them (the
    // random-effect sets' u and varU, the BayesLV sets' c and varZeta) is copied to the plan's offsets here
    const long long nfix = (long long)(pl.size(SEG_FIX) / 8), gap_rand = (long long)(pl.off(SEG_BETA) / 8) - 3 - nfix;
    const long long gap_cls = (long long)((pl.off(SEG_DELTA) - pl.off(SEG_BETA)) / 8) - h->P - h->nvb - 2 * (long long)h->sets.size();
    const long long n = std::max<long long>(std::max<long long>(h->P, h->nvb), std::max<long long>(nfix, 1));
    hipLaunchKernelGGL(k_sample_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, S->d_slot[slot], (long long)h->P, (long long)h->nvb,
                       (int)h->sets.size(), nfix, gap_rand, gap_cls, (long long)h->iter, h->cm.d_beta, h->cm.d_delta, h->mm.d_varBeta, h->cm.d_sets,
                       h->cm.d_scal, h->mm.d_bfix, h->cm.d_abort);
    hipError_t e = hipSuccess;
    for (auto &a : pl.at)
        if (e == hipSuccess && (a.s->id == SEG_U || a.s->id == SEG_VARU || a.s->id == SEG_LV || a.s->id == SEG_RC_PROB || a.s->id == SEG_RC_CAT || a.s->id == SEG_THR_SMP))
            e = hipMemcpyAsync(S->d_slot[slot].get() + a.off, a.s->p, a.s->bytes, hipMemcpyDeviceToDevice, h->stream);
    // (a HIP call that fails here gives the slot back: the next enqueue would otherwise wait for it forever instead of reporting)
    if (e == hipSuccess) e = hipEventRecord(S->ev_packed[slot], h->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(S->copy_stream, S->ev_packed[slot], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(S->h_slot[slot], S->d_slot[slot], S->rec_bytes, hipMemcpyDeviceToHost, S->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(S->ev_copied[slot], S->copy_stream);
    if (e != hipSuccess) {
        { std::lock_guard<std::mutex> lk(S->mu); S->busy[slot] = false; }
        S->cv.notify_all();
        return fail(h, NGP_ERR_HIP, std::string("sample stream: ") + hipGetErrorString(e));
    }
    { std::lock_guard<std::mutex> lk(S->mu); S->queue.push_back(slot); }
    S->cv.notify_all();
    S->nenq++;
    return NGP_OK;
}
// end of a run: every enqueued sample is in the file when the call returns
int sample_flush(ngp_handle *h) {
    SampleStream *S = h->smp.get();
    if (!S) return NGP_OK;
    std::unique_lock<std::mutex> lk(S->mu);
    S->cv.wait(lk, [&] { return S->queue.empty(); });
    if (S->f) std::fflush(S->f.get());
    if (S->io_error) return fail(h, NGP_ERR_ARG, "writing the sample file failed: " + S->path);
    return NGP_OK;
}

// an array and its posterior sums, grown to cap (zeroed) entries with their first n entries kept: varBeta, the fixed effects' b
int grow_pair(ngp_handle *h, DevArray<double> &a, DevArray<double> &sum_a, int64_t n, int64_t cap) {
    DevArray<double> na, ns;
    int rc;
    if ((rc = na.alloc(h, (size_t)cap))) return rc;
    if ((rc = ns.alloc(h, (size_t)cap))) return rc;
    if (n > 0) {
        HCHK(hipMemcpyAsync(na, a, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HCHK(hipMemcpyAsync(ns, sum_a, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    HCHK(hipStreamSynchronize(h->stream));
    a = std::move(na); sum_a = std::move(ns);
    return NGP_OK;
}

// a BayesRCpi set's per-locus state as ngp_add_marker_set_rc leaves it: annotProb[l][a] = annot[l][a] / sum_a annot[l][a]
// (src/mme.jl:395), sum_annot = 0, annotCat = 1.  The reference starts annotCat as zeros(Int64, 1, P) (src/mme.jl:403); nothing reads it
// before the first sweep writes it, and starting at 1 is this library's choice: a valid category from the first get / set on.
int rc_reset(ngp_handle *h, HRc &Rc) {
    std::vector<double> pr((size_t)Rc.A * (size_t)Rc.n, 0.0);
    for (int64_t l = 0; l < Rc.n; l++) {
        const double np = (double)__builtin_popcount((unsigned)Rc.mask[(size_t)l]);
        for (int a = 0; a < Rc.A; a++)
            if ((Rc.mask[(size_t)l] >> a) & 1) pr[(size_t)a * (size_t)Rc.n + (size_t)l] = 1.0 / np;
    }
    HCHK(hipMemcpyAsync(Rc.d_prob, pr.data(), pr.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemsetAsync(Rc.d_cat, 1, (size_t)Rc.n, h->stream));
    HCHK(hipMemsetAsync(Rc.d_sum, 0, pr.size() * sizeof(double), h->stream));
    HCHK(hipStreamSynchronize(h->stream));  // (pr is a local)
    return NGP_OK;
}

// a BayesLV set's state as ngp_add_marker_set_lv leaves it: zeta = zeta0 (or the keyed uniforms), c = 0, varZeta = varZeta0, sums 0
int lv_reset(ngp_handle *h, HLv &V) {
    double st[NGP_LV_WORDS] = {0.0};
    st[NGP_LV_VZ] = V.varZeta0;
    HCHK(hipMemcpyAsync(V.d_st, st, sizeof(st), hipMemcpyHostToDevice, h->stream));
    if (!V.zeta0.empty()) HCHK(hipMemcpyAsync(V.d_zeta, V.zeta0.data(), (size_t)V.n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else hipLaunchKernelGGL(k_lv_start, dim3((unsigned)((V.n + 255) / 256)), dim3(256), 0, h->stream, (long long)V.n, V.d_zeta.get(), V.set, h->seed, (uint64_t)h->chain);
    HCHK(hipStreamSynchronize(h->stream));  // (st is a local)
    return NGP_OK;
}

// BayesLV: inv = inv(C'C + ridge I) of the ncol x nc covariates C (column-major, leading dimension ld), Float64, fixed order:
// (C'C)_ij = sum over the loci in ascending order of C_li C_lj (from 0.0); ridge = min_i |(C'C)_ii / 10000| (src/mme.jl:433-436);
// A = L L' (lower Cholesky, row by row); W = inv(L) by forward substitution, column by column; inv_ij = sum_{k >= max(i, j)} W_ki W_kj
// (ascending k)
int lv_icpc(ngp_handle *h, const double *C, int64_t ld, int64_t ncol, int nc, std::vector<double> &inv) {
    std::vector<double> A((size_t)nc * nc), L((size_t)nc * nc, 0.0), W((size_t)nc * nc, 0.0);
    inv.assign((size_t)nc * nc, 0.0);
    for (int i = 0; i < nc; i++)
        for (int j = 0; j <= i; j++) {
            double a = 0.0;
            for (int64_t l = 0; l < ncol; l++) a = a + C[(size_t)i * ld + l] * C[(size_t)j * ld + l];
            A[(size_t)i * nc + j] = a; A[(size_t)j * nc + i] = a;
        }
    double ridge = std::fabs(A[0] / 10000.0);
    for (int i = 1; i < nc; i++) ridge = std::min(ridge, std::fabs(A[(size_t)i * nc + i] / 10000.0));
    for (int i = 0; i < nc; i++) A[(size_t)i * nc + i] = A[(size_t)i * nc + i] + ridge;
    for (int i = 0; i < nc; i++)
        for (int j = 0; j <= i; j++) {
            double sres = A[(size_t)i * nc + j];
            for (int k = 0; k < j; k++) sres = sres - L[(size_t)i * nc + k] * L[(size_t)j * nc + k];
            if (i == j) {
                REQUIRE(std::isfinite(sres) && sres > 0.0, NGP_ERR_ARG, "BayesLV: C'C (+ ridge) is not positive definite (its Cholesky factorisation fails)");
                L[(size_t)i * nc + i] = std::sqrt(sres);
            } else {
                L[(size_t)i * nc + j] = sres / L[(size_t)j * nc + j];
            }
        }
    for (int j = 0; j < nc; j++)
        for (int i = j; i < nc; i++) {
            double sres = (i == j) ? 1.0 : 0.0;
            for (int k = j; k < i; k++) sres = sres - L[(size_t)i * nc + k] * W[(size_t)k * nc + j];
            W[(size_t)i * nc + j] = sres / L[(size_t)i * nc + i];
        }
    for (int i = 0; i < nc; i++)
        for (int j = 0; j <= i; j++) {
            double a = 0.0;
            for (int k = i; k < nc; k++) a = a + W[(size_t)k * nc + i] * W[(size_t)k * nc + j];
            REQUIRE(std::isfinite(a), NGP_ERR_ARG, "BayesLV: inverting C'C (+ ridge) overflowed");
            inv[(size_t)i * nc + j] = a; inv[(size_t)j * nc + i] = a;
        }
    return NGP_OK;
}

/* ---- adding a marker set.  Every ngp_add_marker_set* is its own argument checks, a MarkerSetSpec, and commit_marker_set ---------- */

struct MarkerSetSpec {
    HSet hs;                     // the host's entry; vb_off = h->nvb: the set's variances follow those of the sets before it
    DSet ds;                     // the device's entry (dset): complete but for pi and the class probabilities, which reset_marker_set writes
    int64_t own0 = 0, own1 = 0;  // the columns [own0, own1) must be free and become the set's; those without a locus are marked -2
    struct Locus { int64_t col; int32_t loc, vb; };
    std::vector<Locus> loci;     // the columns that carry a locus, with their h_loc and h_vbidx
    enum Regions { none, sumsq, tuple } regions = none;  // the table of region draws the set enters: h_regs (a chi-square from a sum of
                                                         // squares), h_tregs (an inverse-Wishart), or neither (BayesB, BayesLV, BayesRCpi)
    const int64_t *reg_start = nullptr, *reg_stop = nullptr;  // its hs.nreg regions, in loci
    const double *lhs0 = nullptr, *rhs0 = nullptr;            // hs.ncol entries each; null: zeros
    // the method's own state, built by its adder and taken over by the commit
    const DTup *tup = nullptr;   // Tuple: its row of d_tup
    HLv *lv = nullptr;           // BayesLV: becomes mm.lv[hs.lv]
    HRc *rc = nullptr;           // BayesRCpi: becomes mm.rc[hs.rc]
};

// one locus per column of the set; locus l takes the variance vb_first + vb_step l
void column_loci(MarkerSetSpec &sp, int64_t vb_first, int64_t vb_step) {
    sp.own0 = sp.hs.col0; sp.own1 = sp.hs.col0 + sp.hs.ncol;
    for (int64_t l = 0; l < sp.hs.ncol; l++) sp.loci.push_back({sp.hs.col0 + l, (int32_t)l, (int32_t)(vb_first + vb_step * l)});
}

DSet dset(int method, int estPi, double df, double scale, int64_t col0, int64_t ncol) {
    DSet ds;
    memset(&ds, 0, sizeof(ds));
    ds.method = method; ds.estPi = estPi; ds.df = df; ds.scale = scale; ds.sdf = scale * df; ds.col0 = col0; ds.ncol = ncol;
    return ds;
}

// May a set take the columns [col0, col0 + span) and own [col0, col0 + owned)?  (A tuple set owns its last 64-column block whole.)
int check_marker_slot(ngp_handle *h, int64_t col0, int64_t span, int64_t owned, const char *outside) {
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->records_only, NGP_ERR_STATE, "this handle has records but no genotype panel (ngp_set_records): it takes no marker sets and sweeps none");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open: x'x and the Gram window exist after ngp_end_panel");
    REQUIRE(h->sets.size() < 16, NGP_ERR_ARG, "at most 16 marker sets");
    REQUIRE(col0 >= 0 && span > 0 && col0 + span <= h->P, NGP_ERR_ARG, outside);
    for (int64_t c = col0; c < std::min<int64_t>(col0 + owned, h->Ppad); c++) REQUIRE(h->h_setof[c] == -1, NGP_ERR_ARG, "marker sets overlap");
    return NGP_OK;
}

// regions must tile [0, n) in order (regionArray of UnitRanges, src/mme.jl:335-347)
int check_regions(ngp_handle *h, const int64_t *reg_start, const int64_t *reg_stop, int64_t nreg, int64_t n, const char *not_covered) {
    int64_t expect = 0;
    for (int64_t r = 0; r < nreg; r++) {
        REQUIRE(reg_start[r] == expect && reg_stop[r] > reg_start[r], NGP_ERR_ARG, "regions must be consecutive and non-empty");
        expect = reg_stop[r];
    }
    REQUIRE(expect == n, NGP_ERR_ARG, not_covered);
    return NGP_OK;
}

int check_classes(ngp_handle *h, const std::string &method, const double *vClass, const double *pi, int K) {
    double ps = 0.0;
    for (int v = 0; v < K; v++) {
        REQUIRE(std::isfinite(vClass[v]) && vClass[v] >= 0.0 && std::isfinite(pi[v]) && pi[v] > 0.0, NGP_ERR_ARG,
                method + ": class multipliers must be >= 0 and class probabilities > 0");
        ps += pi[v];
    }
    REQUIRE(std::fabs(ps - 1.0) < 1e-8, NGP_ERR_ARG, method + ": class probabilities must sum to 1");
    return NGP_OK;
}

// A set as a chain starts from it: the variances, pi and the class probabilities at their prior values, empty pi sums (src/mme.jl:351-360,
// 374-383, 516).  The commit of a new set and ngp_set_y both come here: a set starts the way it restarts.  Device only; hs is the set's
// entry, which the commit has not stored yet.
int reset_marker_set(ngp_handle *h, int si, const HSet &hs) {
    HCHK(hipMemcpyAsync(h->mm.d_varBeta + hs.vb_off, hs.vb0.data(), hs.vb0.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_set_pi, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, si, 1.0 - hs.pi0, hs.pi0);
    hipLaunchKernelGGL(k_set_sum_pi, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, si, 0.0, 0.0);
    if (hs.K > 0) return set_class_state_dev(h, si, hs.K, hs.rpi.data(), std::vector<double>((size_t)hs.K, 0.0).data());
    return NGP_OK;
}

// the variance segments (at most NGP_SEG loci each) of the region [start, stop) of set si, appended to a segment table; rg: its entry
template <typename Reg>
void push_region(Reg &rg, int64_t first, int64_t start, int64_t stop, int si, std::vector<long long> &seg_first, std::vector<int32_t> &seg_len,
                 std::vector<int32_t> &seg_set) {
    rg.seg0 = (long long)seg_first.size(); rg.set = si; rg.n = stop - start; rg.nseg = 0;
    for (int64_t l0 = start; l0 < stop; l0 += NGP_SEG) {
        seg_first.push_back(first + l0);
        seg_len.push_back((int32_t)std::min<int64_t>(NGP_SEG, stop - l0));
        seg_set.push_back((int32_t)si);
        rg.nseg++;
    }
}

/* The one way a marker set enters the handle.  Phase 1 is everything that can fail -- host and device memory, every upload and launch
 * -- and writes only where no reader looks before phase 2: behind nvb, at d_sets[si] and the method's tables of a set that does not
 * exist yet, over columns no set owns.  Phase 2 makes the set exist in the host tables and cannot fail.  A refused or failed add
 * therefore leaves the handle as it was. */
int commit_marker_set(ngp_handle *h, MarkerSetSpec &sp, int32_t *set_id) {
    int rc;
    const HSet &hs = sp.hs;
    const int si = (int)h->sets.size();
    const int64_t new_nvb = h->nvb + (int64_t)hs.vb0.size();
    // ---- phase 1 ----
    size_t nseg = 0;
    for (int64_t r = 0; sp.regions != MarkerSetSpec::none && r < hs.nreg; r++) nseg += (size_t)((sp.reg_stop[r] - sp.reg_start[r] + NGP_SEG - 1) / NGP_SEG);
    h->sets.reserve(h->sets.size() + 1);
    if (sp.regions == MarkerSetSpec::sumsq) {
        h->h_regs.reserve(h->h_regs.size() + (size_t)hs.nreg);
        for (auto *v : {&h->h_seg_len, &h->h_seg_set}) v->reserve(v->size() + nseg);
        h->h_seg_k0.reserve(h->h_seg_k0.size() + nseg);
    } else if (sp.regions == MarkerSetSpec::tuple) {
        h->h_tregs.reserve(h->h_tregs.size() + (size_t)hs.nreg);
        for (auto *v : {&h->h_tseg_len, &h->h_tseg_set}) v->reserve(v->size() + nseg);
        h->h_tseg_l0.reserve(h->h_tseg_l0.size() + nseg);
    }
    if (sp.lv) h->mm.lv.reserve(h->mm.lv.size() + 1);
    if (sp.rc) h->mm.rc.reserve(h->mm.rc.size() + 1);
    if (new_nvb > h->mm.vb_cap) {
        const int64_t cap = std::max<int64_t>(new_nvb, 2 * h->mm.vb_cap);
        if ((rc = grow_pair(h, h->mm.d_varBeta, h->mm.d_sum_varBeta, h->nvb, cap))) return rc;
        h->mm.vb_cap = cap;
    }
    if (hs.K > 0 && !h->mm.d_rcls && (rc = h->mm.d_rcls.alloc(h, (size_t)4 * NGP_RMAX * (size_t)h->Ppad))) return rc;
    if (sp.rc && !h->mm.d_rctab && (rc = h->mm.d_rctab.alloc(h, 16))) return rc;
    if (sp.tup) {
        if (!h->mm.d_tup && (rc = h->mm.d_tup.alloc(h, 16))) return rc;
        if (!h->mm.d_tupc && (rc = h->mm.d_tupc.alloc(h, (size_t)NGP_KMAX * (size_t)h->Ppad))) return rc;
        if (!h->mm.d_tupg && (rc = h->mm.d_tupg.alloc(h, (size_t)NGP_KMAX * (size_t)h->Ppad))) return rc;
    }
    const std::vector<double> z((size_t)((sp.lhs0 && sp.rhs0) ? 0 : hs.ncol), 0.0);
    HCHK(hipMemcpyAsync(h->cm.d_lhs0 + hs.col0, sp.lhs0 ? sp.lhs0 : z.data(), (size_t)hs.ncol * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(h->cm.d_rhs0 + hs.col0, sp.rhs0 ? sp.rhs0 : z.data(), (size_t)hs.ncol * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(h->cm.d_sets + si, &sp.ds, sizeof(DSet), hipMemcpyHostToDevice, h->stream));
    DRc dr;
    if (sp.rc) {
        dr = sp.rc->dev();
        HCHK(hipMemcpyAsync(h->mm.d_rctab + si, &dr, sizeof(DRc), hipMemcpyHostToDevice, h->stream));
    }
    if (sp.tup) {
        HCHK(hipMemcpyAsync(h->mm.d_tup + si, sp.tup, sizeof(DTup), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_tuple_gkk, dim3((unsigned)((sp.tup->nloc * sp.tup->k + 255) / 256)), dim3(256), 0, h->stream, h->pm->gramx, h->plan.D, h->pm->mpm,
                           *sp.tup, h->mm.d_tupg, (long long)h->Ppad);
    }
    if ((rc = reset_marker_set(h, si, hs))) return rc;
    HCHK(hipStreamSynchronize(h->stream));  // (the sources of the copies are the caller's, sp's and this function's locals)
    // ---- phase 2 ----
    std::fill(h->h_setof.begin() + sp.own0, h->h_setof.begin() + sp.own1, (int8_t)-2);
    for (const MarkerSetSpec::Locus &l : sp.loci) {
        h->h_setof[l.col] = (int8_t)si;
        h->h_loc[l.col] = l.loc;
        h->h_vbidx[l.col] = l.vb;
    }
    for (int64_t r = 0; sp.regions != MarkerSetSpec::none && r < hs.nreg; r++) {
        if (sp.regions == MarkerSetSpec::sumsq) {
            DReg dg;
            dg.rg = (int)r; dg.vb = (int)(hs.vb_off + r);
            push_region(dg, hs.col0, sp.reg_start[r], sp.reg_stop[r], si, h->h_seg_k0, h->h_seg_len, h->h_seg_set);
            h->h_regs.push_back(dg);
        } else {
            DTReg tg;
            tg.rg = r;
            push_region(tg, 0, sp.reg_start[r], sp.reg_stop[r], si, h->h_tseg_l0, h->h_tseg_len, h->h_tseg_set);
            h->h_tregs.push_back(tg);
        }
    }
    h->nvb = new_nvb;
    h->nclass_total += hs.K;
    if (sp.tup) h->ntuple += 1;
    if (sp.lv) h->mm.lv.push_back(std::move(*sp.lv));
    if (sp.rc) h->mm.rc.push_back(std::move(*sp.rc));
    h->sets.push_back(std::move(sp.hs));
    h->tables_dirty = true;
    h->mm.trace_ext_cap = 0;  // d_tr_pi holds one column per set: sized again by the next traced ngp_run
    if (set_id) *set_id = si;
    return NGP_OK;
}

int ready(ngp_handle *h) {
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open: ngp_end_panel builds the Gram window the sweep needs");
    REQUIRE(h->have_y, NGP_ERR_STATE, "y not set");
    // (a records-only handle with a hold-out set may be the intercept-only model y = b + e: the closed-form case of the augmentation step)
    // (... and so may one with liability traits: the intercept-only probit and Tobit models)
    if (h->records_only) REQUIRE(!h->mm.rnd.empty() || (h->intercept && (!h->cm.ho_rows.empty() || h->cm.lb.on())), NGP_ERR_STATE,
                                 "no random-effect set added (a handle made by ngp_set_records has no marker sets)");
    else REQUIRE(!h->sets.empty(), NGP_ERR_STATE, "no marker set added");
    int rc;
    if ((rc = sync_tables(h))) return rc;
    return sync_linear_blocks(h, -1);
}

}  // namespace

extern "C" {

int32_t ngp_abi_version(void) { return NGP_ABI_VERSION; }

int32_t ngp_create(int32_t device, uint64_t seed, uint32_t chain_id, ngp_handle **out) {
    NGP_TRY
    if (!out) return fail(nullptr, NGP_ERR_ARG, "null out pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, NGP_ERR_NODEVICE, std::string("no HIP device available (") + hipGetErrorString(e) +
                                                   "); libnextgp_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, NGP_ERR_ARG, "device index out of range");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(nullptr, NGP_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, NGP_ERR_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    ngp_handle *h = new (std::nothrow) ngp_handle();
    if (!h) return fail(nullptr, NGP_ERR_NOMEM, "out of host memory");
    h->device = device; h->seed = seed; h->chain = chain_id; h->cu_count = prop.multiProcessorCount;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreate(&h->stream)) != hipSuccess ||
        (e = hipEventCreate(&h->ev0)) != hipSuccess || (e = hipEventCreate(&h->ev1)) != hipSuccess) {
        std::string m = std::string("ngp_create: ") + hipGetErrorString(e);
        delete h;
        return fail(nullptr, NGP_ERR_HIP, m);
    }
    *out = h;
    return NGP_OK;
    NGP_CATCH(nullptr)
}

int32_t ngp_destroy(ngp_handle *h) {
    NGP_TRY
    if (!h) return NGP_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->smp.reset();  // (stops the sample writer; the device arrays go with the handle)
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return NGP_OK;
    NGP_CATCH(h)
}

const char *ngp_last_error(ngp_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int32_t ngp_set_panel_f64(ngp_handle *h, const double *M, int64_t N, int64_t P, int64_t ld, int32_t centre) {
    NGP_TRY
    return set_panel_host<double>(h, M, N, P, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_set_panel_f32(ngp_handle *h, const float *M, int64_t N, int64_t P, int64_t ld, int32_t centre) {
    NGP_TRY
    return set_panel_host<float>(h, M, N, P, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_begin_panel(ngp_handle *h, int64_t N, int64_t P) {
    NGP_TRY
    return begin_panel(h, N, P);
    NGP_CATCH(h)
}
int32_t ngp_panel_columns_f64(ngp_handle *h, int64_t col0, const double *M, int64_t ncol, int64_t ld, int32_t centre) {
    NGP_TRY
    return panel_columns<double>(h, col0, M, ncol, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_panel_columns_f32(ngp_handle *h, int64_t col0, const float *M, int64_t ncol, int64_t ld, int32_t centre) {
    NGP_TRY
    return panel_columns<float>(h, col0, M, ncol, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_panel_columns_u8(ngp_handle *h, int64_t col0, const uint8_t *G, int64_t ncol, int64_t ld, int32_t centre) {
    NGP_TRY
    return panel_columns<uint8_t>(h, col0, G, ncol, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_end_panel(ngp_handle *h) {
    NGP_TRY
    return end_panel(h);
    NGP_CATCH(h)
}

}  // extern "C" (helpers below are C++)

// one staged chunk of genotype bytes (whole 64-column blocks, column-major with leading dimension ld, already on the device)
// into the tiles: fp32 centred tiles, or the bytes as they are plus the column means (compact storage)
static void ingest_u8_chunk(ngp_handle *h, const uint8_t *d_g, int64_t N, int64_t ld, int64_t t0, int64_t nb, int64_t ncols, int centre,
                            double *d_mu) {
    const int64_t c0 = t0 * NGP_BLK;
    if (h->req.storage == 1) {  // the bytes stay bytes; the means go to the handle
        hipLaunchKernelGGL(k_u8_colmean, dim3((unsigned)ncols), dim3(256), 0, h->stream, d_g, (long long)N, (long long)ld, (int)centre,
                           h->pm->mean + c0);
        hipLaunchKernelGGL(k_u8_fill8, dim3((unsigned)h->plan.S, (unsigned)nb), dim3(256), 0, h->stream, (uint8_t *)h->pm->tiles.get(), d_g, (long long)N,
                           (long long)ld, (long long)ncols, (int)h->plan.R, (int)h->plan.S, (long long)t0);
    } else {
        hipLaunchKernelGGL(k_u8_colmean, dim3((unsigned)ncols), dim3(256), 0, h->stream, d_g, (long long)N, (long long)ld, (int)centre, d_mu);
        (void)hipMemcpyAsync(h->pm->mean + c0, d_mu, (size_t)ncols * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        hipLaunchKernelGGL(k_u8_fill, dim3((unsigned)h->plan.S, (unsigned)nb), dim3(256), 0, h->stream, h->pm->tiles, d_g, (long long)N,
                           (long long)ld, (long long)ncols, (int)h->plan.R, (int)h->plan.S, (long long)t0, d_mu, (const double *)h->cm.d_rs);
    }
}

extern "C" {

int32_t ngp_set_panel_u8(ngp_handle *h, const uint8_t *G, int64_t N, int64_t P, int64_t ld, int32_t centre) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(G != nullptr, NGP_ERR_ARG, "null panel pointer");
    REQUIRE(ld >= N, NGP_ERR_ARG, "leading dimension smaller than N");
    if ((rc = alloc_panel(h, N, P))) return rc;
    // staged through the device in chunks of whole 64-column blocks (about 64 MiB of genotypes at a time)
    const int64_t blk_bytes = (int64_t)NGP_BLK * ld;
    const int64_t nb_chunk = std::max<int64_t>(1, std::min<int64_t>(h->NBLK, staging_bytes(h, (int64_t)64 << 20) / blk_bytes));
    DevArray<uint8_t> d_g;
    DevArray<double> d_mu;
    if (d_g.alloc_raw((size_t)nb_chunk * blk_bytes) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "staging buffer");
    if ((rc = d_mu.alloc(h, (size_t)nb_chunk * NGP_BLK))) return rc;
    hipError_t e = hipSuccess;
    for (int64_t t0 = 0; t0 < h->NBLK && e == hipSuccess; t0 += nb_chunk) {
        const int64_t nb = std::min<int64_t>(nb_chunk, h->NBLK - t0);
        const int64_t c0 = t0 * NGP_BLK, ncols = std::min<int64_t>(nb * NGP_BLK, P - c0);
        // the last column may be shorter than ld in the caller's buffer: copy ncols-1 full columns + N bytes
        const size_t bytes = (size_t)(ncols - 1) * ld + (size_t)N;
        e = hipMemcpyAsync(d_g, G + (size_t)c0 * ld, bytes, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) break;
        ingest_u8_chunk(h, d_g, N, ld, t0, nb, ncols, centre, d_mu);
        e = hipStreamSynchronize(h->stream);  // the staging buffer is reused by the next chunk
    }
    d_g.reset(); d_mu.reset();  // (before the Gram window's scratch is allocated)
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("set_panel_u8: ") + hipGetErrorString(e));
    return build_gram(h);
    NGP_CATCH(h)
}

// ---- binary panel file (replaces the text genotype file of src/prepMatVec.jl:116-131 for large panels) ----
// header (32 bytes): magic "NGPPNL01", int64 N, int64 P, int32 bits (8 or 2), int32 0.  Then P columns: N bytes (bits 8), or
// ceil(N / 4) bytes with four genotypes per byte, individual i in bits 2 (i mod 4) .. 2 (i mod 4) + 1 (bits 2; code 3 is refused).
namespace {
struct PanelHeader { char magic[8]; int64_t N, P; int32_t bits, zero; };
}
#define NGP_SNAP_WEIGHTED ((int64_t)1 << 62)  // snapshot: the fixed-set count's flag of a weighted chain (ngp_save_snapshot)
#define NGP_SNAP_RANDOM ((int64_t)1 << 61)    // ... and of a chain with random-effect sets
#define NGP_SNAP_HOLDOUT ((int64_t)1 << 60)   // ... and of a chain with held-out records (ngp_set_holdout)
#define NGP_SNAP_LIABILITY ((int64_t)1 << 59) // ... of a chain with liability traits (ngp_set_liability_classes / ngp_set_liability_bounds)
#define NGP_SNAP_FIXVARE ((int64_t)1 << 58)   // ... and of a chain whose residual variance is held fixed (ngp_fix_residual_variance)
// snapshot signature of a BayesLV set (added to its second word): the covariate count and how varZeta is estimated
static int64_t lv_sig(const ngp_handle *h, const HSet &hs) {
    return hs.lv < 0 ? 0 : 256 * ((int64_t)h->mm.lv[(size_t)hs.lv].ncov + 32 * (int64_t)h->mm.lv[(size_t)hs.lv].mode);
}

// ... and of a BayesRCpi set: 47 bits of a digest (FNV-1a) of its annotation masks from bit 8 up -- a snapshot's annotProb is positive
// exactly where the mask it was saved under has a bit, so it may only load into a model with the same annotations
static int64_t rc_sig(const ngp_handle *h, const HSet &hs) {
    if (hs.rc < 0) return 0;
    uint64_t d = 1469598103934665603ull;
    for (uint8_t m : h->mm.rc[(size_t)hs.rc].mask) { d ^= m; d *= 1099511628211ull; }
    return (int64_t)((d >> 17) << 8);
}

int32_t ngp_write_panel_file(const char *path, const uint8_t *G, int64_t N, int64_t P, int64_t ld, int32_t bits) {
    NGP_TRY
    if (!path || !G || N <= 0 || P <= 0 || ld < N || (bits != 8 && bits != 2)) return NGP_ERR_ARG;
    std::vector<uint8_t> packed(bits == 2 ? (size_t)(N + 3) / 4 : 0);  // before the file is opened: an allocation failure leaves nothing behind
    File f(std::fopen(path, "wb"));
    if (!f) return NGP_ERR_ARG;
    PanelHeader hd;
    std::memcpy(hd.magic, "NGPPNL01", 8);
    hd.N = N; hd.P = P; hd.bits = bits; hd.zero = 0;
    bool ok = std::fwrite(&hd, sizeof hd, 1, f.get()) == 1;
    for (int64_t j = 0; j < P && ok; j++) {
        const uint8_t *col = G + (size_t)j * ld;
        if (bits == 8) {
            ok = std::fwrite(col, 1, (size_t)N, f.get()) == (size_t)N;
        } else {
            std::fill(packed.begin(), packed.end(), 0);
            for (int64_t i = 0; i < N; i++) {
                if (col[i] > 2) { ok = false; break; }  // two bits hold the allele counts 0, 1, 2
                packed[(size_t)i >> 2] |= (uint8_t)(col[i] << (2 * (i & 3)));
            }
            if (ok) ok = std::fwrite(packed.data(), 1, packed.size(), f.get()) == packed.size();
        }
    }
    ok = (std::fclose(f.release()) == 0) && ok;  // (a failed close is a failed write)
    return ok ? NGP_OK : NGP_ERR_ARG;
    NGP_CATCH(nullptr)
}

int32_t ngp_read_panel_header(const char *path, int64_t *N, int64_t *P, int32_t *bits) {
    NGP_TRY
    if (!path) return NGP_ERR_ARG;
    File f(std::fopen(path, "rb"));
    if (!f) return NGP_ERR_ARG;
    PanelHeader hd;
    const bool ok = std::fread(&hd, sizeof hd, 1, f.get()) == 1 && std::memcmp(hd.magic, "NGPPNL01", 8) == 0 && hd.N > 0 && hd.P > 0 &&
                    (hd.bits == 8 || hd.bits == 2);
    if (!ok) return NGP_ERR_ARG;
    if (N) *N = hd.N;
    if (P) *P = hd.P;
    if (bits) *bits = hd.bits;
    return NGP_OK;
    NGP_CATCH(nullptr)
}

int32_t ngp_load_panel_file(ngp_handle *h, const char *path, int32_t centre) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(path != nullptr, NGP_ERR_ARG, "null path");
    File f(std::fopen(path, "rb"));
    REQUIRE(f != nullptr, NGP_ERR_ARG, std::string("cannot open panel file ") + path);
    PanelHeader hd;
    if (std::fread(&hd, sizeof hd, 1, f.get()) != 1 || std::memcmp(hd.magic, "NGPPNL01", 8) != 0 || hd.N <= 0 || hd.P <= 0 || (hd.bits != 8 && hd.bits != 2))
        return fail(h, NGP_ERR_ARG, std::string("not a panel file (magic NGPPNL01, bits 8 or 2): ") + path);
    const int64_t N = hd.N, P = hd.P;
    if ((rc = alloc_panel(h, N, P))) return rc;
    // the file streams through a pinned host buffer in chunks of whole 64-column blocks; two-bit columns are unpacked on the host
    const int64_t colbytes = (hd.bits == 8) ? N : (N + 3) / 4;
    const int64_t blk_bytes = (int64_t)NGP_BLK * N;
    const int64_t nb_chunk = std::max<int64_t>(1, std::min<int64_t>(h->NBLK, staging_bytes(h, (int64_t)64 << 20) / blk_bytes));
    DevArray<uint8_t> d_g;
    PinnedArray<uint8_t> h_g;
    DevArray<double> d_mu;
    std::vector<uint8_t> packed((hd.bits == 2) ? (size_t)colbytes : 0);
    hipError_t e = d_g.alloc_raw((size_t)nb_chunk * blk_bytes);
    if (e == hipSuccess) e = h_g.alloc_raw((size_t)nb_chunk * blk_bytes);
    if (e != hipSuccess) return fail(h, NGP_ERR_NOMEM, "staging buffers");
    if ((rc = d_mu.alloc(h, (size_t)nb_chunk * NGP_BLK))) return rc;
    std::string why;
    for (int64_t t0 = 0; t0 < h->NBLK && e == hipSuccess && why.empty(); t0 += nb_chunk) {
        const int64_t nb = std::min<int64_t>(nb_chunk, h->NBLK - t0);
        const int64_t c0 = t0 * NGP_BLK, ncols = std::min<int64_t>(nb * NGP_BLK, P - c0);
        for (int64_t jc = 0; jc < ncols && why.empty(); jc++) {
            uint8_t *dst = h_g + (size_t)jc * N;
            if (hd.bits == 8) {
                if (std::fread(dst, 1, (size_t)N, f.get()) != (size_t)N) why = "panel file truncated";
            } else {
                if (std::fread(packed.data(), 1, packed.size(), f.get()) != packed.size()) { why = "panel file truncated"; break; }
                for (int64_t i = 0; i < N; i++) {
                    const uint8_t g = (uint8_t)((packed[(size_t)i >> 2] >> (2 * (i & 3))) & 3u);
                    if (g == 3) { why = "panel file holds a missing genotype (code 3): impute before loading"; break; }
                    dst[i] = g;
                }
            }
        }
        if (!why.empty()) break;
        e = hipMemcpyAsync(d_g, h_g, (size_t)ncols * N, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) break;
        ingest_u8_chunk(h, d_g, N, N, t0, nb, ncols, centre, d_mu);
        e = hipStreamSynchronize(h->stream);  // both staging buffers are reused by the next chunk
    }
    f.reset(); d_g.reset(); h_g.reset(); d_mu.reset();  // (before the Gram window's scratch is allocated)
    if (!why.empty()) { drop_panel(h); return fail(h, NGP_ERR_ARG, why); }
    if (e != hipSuccess) { drop_panel(h); return fail(h, NGP_ERR_HIP, std::string("load_panel_file: ") + hipGetErrorString(e)); }
    return build_gram(h);
    NGP_CATCH(h)
}

int32_t ngp_generate_panel(ngp_handle *h, int64_t N, int64_t P, double maf_lo, double maf_hi, uint64_t panel_seed) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(maf_lo > 0.0 && maf_hi < 1.0 && maf_lo <= maf_hi, NGP_ERR_ARG, "maf range must satisfy 0 < lo <= hi < 1");
    const auto ts0 = std::chrono::steady_clock::now();
    if ((rc = alloc_panel(h, N, P))) return rc;
    (void)hipStreamSynchronize(h->stream);  // (the allocations' zeroing: timed with them)
    const auto ts1 = std::chrono::steady_clock::now();
    DevArray<double> d_mu;
    DevArray<uint32_t> d_thr;
    if ((rc = d_mu.alloc(h, (size_t)P))) return rc;
    if ((rc = d_thr.alloc(h, (size_t)P))) return rc;
    hipLaunchKernelGGL(k_gen_colmean, dim3((unsigned)P), dim3(256), 0, h->stream, (long long)N, (long long)P, maf_lo, maf_hi, panel_seed,
                       d_mu, d_thr);
    (void)hipMemcpyAsync(h->pm->mean, d_mu, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
    if (h->req.storage == 1) {
        hipLaunchKernelGGL(k_gen_fill8, dim3((unsigned)h->plan.S, (unsigned)h->NBLK), dim3(256), 0, h->stream, (uint8_t *)h->pm->tiles.get(), (long long)N,
                           (long long)P, (int)h->plan.R, (int)h->plan.S, panel_seed, d_thr);
    } else
    hipLaunchKernelGGL(k_gen_fill, dim3((unsigned)h->plan.S, (unsigned)h->NBLK), dim3(256), 0, h->stream, h->pm->tiles, (long long)N,
                       (long long)P, (int)h->plan.R, (int)h->plan.S, panel_seed, d_mu, d_thr, (const double *)h->cm.d_rs);
    hipError_t e = hipStreamSynchronize(h->stream);
    d_mu.reset(); d_thr.reset();  // (before the Gram window's scratch is allocated)
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("generate_panel: ") + hipGetErrorString(e));
    const auto ts2 = std::chrono::steady_clock::now();
    rc = build_gram(h);
    const auto ts3 = std::chrono::steady_clock::now();
    h->setup_ms[0] = std::chrono::duration<double, std::milli>(ts1 - ts0).count();
    h->setup_ms[1] = std::chrono::duration<double, std::milli>(ts2 - ts1).count();
    h->setup_ms[2] = std::chrono::duration<double, std::milli>(ts3 - ts2).count();
    return rc;
    NGP_CATCH(h)
}

int32_t ngp_get_setup_timing(ngp_handle *h, double *alloc_ms, double *tiles_ms, double *gram_ms) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (alloc_ms) *alloc_ms = h->setup_ms[0];
    if (tiles_ms) *tiles_ms = h->setup_ms[1];
    if (gram_ms) *gram_ms = h->setup_ms[2];
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_layout(ngp_handle *h, int64_t *R, int64_t *S, int64_t *nblk) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    if (R) *R = h->plan.R;
    if (S) *S = h->plan.S;
    if (nblk) *nblk = h->NBLK;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_mpm(ngp_handle *h, double *out, int64_t P) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open: x'x and the Gram window exist after ngp_end_panel");
    REQUIRE(out && P == h->P, NGP_ERR_ARG, "mpm buffer must hold P entries");
    HCHK(hipMemcpy(out, h->pm->mpm, (size_t)P * sizeof(double), hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_gram(ngp_handle *h, int64_t t, double *out) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open: x'x and the Gram window exist after ngp_end_panel");
    REQUIRE(out && t >= 0 && t < h->NBLK, NGP_ERR_ARG, "block index out of range");
    HCHK(hipMemcpy(out, h->pm->gramx + (size_t)t * h->plan.D * NGP_BLK * NGP_BLK, NGP_BLK * NGP_BLK * sizeof(double), hipMemcpyDeviceToHost));
    // the device keeps entry [k][j] for j > k only (plus x'x in mpm); hand back the symmetric block
    double diag[NGP_BLK];
    HCHK(hipMemcpy(diag, h->pm->mpm + (size_t)t * NGP_BLK, sizeof(diag), hipMemcpyDeviceToHost));
    for (int k = 0; k < NGP_BLK; k++) {
        out[k * NGP_BLK + k] = diag[k];
        for (int j = k + 1; j < NGP_BLK; j++) out[j * NGP_BLK + k] = out[k * NGP_BLK + j];
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_xbeta(ngp_handle *h, const double *beta, int64_t P, double *out, int64_t N) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open: x'x and the Gram window exist after ngp_end_panel");
    REQUIRE(beta && out && P == h->P && N == h->N, NGP_ERR_ARG, "xbeta: size mismatch");
    DevArray<double> d_b, d_o;
    if ((rc = d_b.alloc(h, (size_t)h->Ppad))) return rc;
    if ((rc = d_o.alloc(h, (size_t)h->L))) return rc;
    hipError_t e = hipMemcpyAsync(d_b, beta, (size_t)P * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && (size_t)h->Ppad > (size_t)P) e = hipMemsetAsync(d_b + P, 0, ((size_t)h->Ppad - (size_t)P) * sizeof(double), h->stream);
    if (h->req.storage == 1)
        hipLaunchKernelGGL(k_xbeta8, dim3((unsigned)h->plan.S), dim3(256), 0, h->stream, (const uint8_t *)h->pm->tiles.get(), h->pm->mean, d_b, d_o, (int)h->plan.R,
                           (int)h->plan.S, (long long)h->NBLK, (long long)h->N);
    else
    hipLaunchKernelGGL(k_xbeta, dim3((unsigned)h->plan.S), dim3(256), 0, h->stream, h->pm->tiles, d_b, d_o, (int)h->plan.R, (int)h->plan.S,
                       (long long)h->NBLK);
    if (h->cm.d_rs) launch_rows(h, d_o, d_o, true);  // the tiles hold s x: X beta = (X~ beta) / s
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_o, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("xbeta: ") + hipGetErrorString(e));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_add_marker_set(ngp_handle *h, int64_t col0, int64_t ncol, int32_t method, double df, double scale,
                           const int64_t *reg_start, const int64_t *reg_stop, int64_t nreg, const double *varBeta0, double pi0,
                           int32_t estPi, const double *lhs0, const double *rhs0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = check_marker_slot(h, col0, ncol, ncol, "marker set outside the panel"))) return rc;
    REQUIRE(method == NGP_METHOD_BAYESPR || method == NGP_METHOD_BAYESB || method == NGP_METHOD_BAYESC || method == NGP_METHOD_BAYESR, NGP_ERR_ARG,
            "unknown method");
    REQUIRE(method != NGP_METHOD_BAYESR, NGP_ERR_ARG, "BayesR sets are added with ngp_add_marker_set_r (classes and their probabilities)");
    REQUIRE(reg_start && reg_stop && varBeta0 && nreg > 0, NGP_ERR_ARG, "regions / varBeta0 missing");
    REQUIRE(std::isfinite(df) && std::isfinite(scale) && df > 0, NGP_ERR_ARG, "df/scale must be finite, df > 0");
    if (method == NGP_METHOD_BAYESB) {
        REQUIRE(nreg == ncol, NGP_ERR_ARG, "BayesB needs one region per locus (src/mme.jl:356)");
        REQUIRE(pi0 > 0.0 && pi0 < 1.0, NGP_ERR_ARG, "BayesB pi must be in (0,1)");
    }
    if (method == NGP_METHOD_BAYESC) {
        REQUIRE(nreg == 1, NGP_ERR_ARG, "BayesC has one variance for the whole set (src/functions.jl:205)");
        REQUIRE(pi0 > 0.0 && pi0 < 1.0, NGP_ERR_ARG, "BayesC pi must be in (0,1)");
        REQUIRE(varBeta0[0] > 0.0, NGP_ERR_ARG, "BayesC varBeta0 must be positive");
    }
    if ((rc = check_regions(h, reg_start, reg_stop, nreg, ncol, "regions must cover the whole set"))) return rc;
    for (int64_t r = 0; r < nreg; r++) REQUIRE(std::isfinite(varBeta0[r]) && varBeta0[r] >= 0.0, NGP_ERR_ARG, "varBeta0 must be finite and >= 0");
    MarkerSetSpec sp;
    sp.hs = HSet{col0, ncol, method, df, scale, nreg, h->nvb, estPi, 0, pi0, std::vector<double>(varBeta0, varBeta0 + nreg)};
    sp.ds = dset(method, estPi, df, scale, col0, ncol);
    sp.own0 = col0; sp.own1 = col0 + ncol;
    for (int64_t r = 0; r < nreg; r++)  // BayesB: a variance per locus; BayesPR, BayesC: one per region
        for (int64_t l = reg_start[r]; l < reg_stop[r]; l++)
            sp.loci.push_back({col0 + l, (int32_t)l, (int32_t)(h->nvb + (method == NGP_METHOD_BAYESB ? l : r))});
    if (method != NGP_METHOD_BAYESB) sp.regions = MarkerSetSpec::sumsq;  // sets whose variance comes from a sum of squares
    sp.reg_start = reg_start; sp.reg_stop = reg_stop;
    sp.lhs0 = lhs0; sp.rhs0 = rhs0;
    return commit_marker_set(h, sp, set_id);
    NGP_CATCH(h)
}

int32_t ngp_set_y(ngp_handle *h, const double *y, int64_t N) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(y && N == h->N, NGP_ERR_ARG, "y must have N entries");
    std::vector<double> y_lb;  // liability traits: y with the starting liability on every augmented row (classes: y is read nowhere)
    if ((rc = start_liabilities(h, y, y_lb))) return rc;
    if (!y_lb.empty()) y = y_lb.data();
    const std::vector<long long> &ho = h->cm.ho_rows;
    std::vector<double> y_aug;  // held-out records: y with the mean of the observed phenotypes on the held-out rows, which are not read
    if (ho.empty()) {
        for (int64_t i = 0; i < N; i++) REQUIRE(std::isfinite(y[i]), NGP_ERR_ARG, "non-finite phenotype");
    } else {
        double sum_obs = 0.0;
        size_t k = 0;
        for (int64_t i = 0; i < N; i++) {
            if (k < ho.size() && ho[k] == i) { k++; continue; }
            REQUIRE(std::isfinite(y[i]), NGP_ERR_ARG, "non-finite phenotype");
            sum_obs = sum_obs + y[i];  // index order, left to right
        }
        const double ybar = sum_obs / (double)(N - (int64_t)ho.size());
        y_aug.assign(y, y + N);
        for (long long i : ho) y_aug[(size_t)i] = ybar;
        y = y_aug.data();
        const std::vector<double> ya(ho.size(), ybar);
        const size_t N8 = (size_t)N * sizeof(double);
        HCHK(hipMemcpy(h->cm.d_yaug, ya.data(), ya.size() * sizeof(double), hipMemcpyHostToDevice));
        HCHK(hipMemsetAsync(h->cm.d_sum_fit, 0, N8, h->stream));
        HCHK(hipMemsetAsync(h->cm.d_sum_fit2, 0, N8, h->stream));
        HCHK(hipMemsetAsync(h->cm.d_n_fit, 0, N8, h->stream));
    }
    HCHK(hipMemsetAsync(h->cm.d_ycorr, 0, (size_t)h->L * sizeof(double), h->stream));
    HCHK(hipMemcpyAsync(h->cm.d_ycorr, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, h->stream));  // src/mme.jl:57
    if (!y_aug.empty() || !y_lb.empty()) HCHK(hipStreamSynchronize(h->stream));  // (the copy reads y_aug / y_lb)
    if (h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, false);  // weighted residuals: y~ = s y
    HCHK(hipMemsetAsync(h->cm.d_beta, 0, (size_t)h->Ppad * sizeof(double), h->stream));                  // src/mme.jl:443
    HCHK(hipMemsetAsync(h->cm.d_delta, 1, (size_t)h->Ppad, h->stream));                                  // src/mme.jl:444
    HCHK(hipMemsetAsync(h->cm.d_scal, 0, sizeof(DScal), h->stream));
    if (h->fix_varE > 0.0) hipLaunchKernelGGL(k_set_varE, dim3(1), dim3(1), 0, h->stream, h->cm.d_scal, h->fix_varE);  // held from here on
    HCHK(hipMemsetAsync(h->cm.d_sum_beta, 0, (size_t)h->Ppad * sizeof(double), h->stream));
    HCHK(hipMemsetAsync(h->cm.d_sum_beta2, 0, (size_t)h->Ppad * sizeof(double), h->stream));
    HCHK(hipMemsetAsync(h->cm.d_sum_delta, 0, (size_t)h->Ppad * sizeof(double), h->stream));
    if ((rc = ensure_prediction(h, true))) return rc;  // the prediction sums are zeroed wherever sum_beta is
    if ((rc = ensure_genvar(h, true))) return rc;      // ... and the genomic-variance sums
    if ((rc = ensure_diag(h, true))) return rc;        // ... and the convergence diagnostics
    // a second chain on the same handle starts from the priors, with empty posterior sums (src/mme.jl:351-360, 516)
    if (h->nvb > 0) HCHK(hipMemsetAsync(h->mm.d_sum_varBeta, 0, (size_t)h->nvb * sizeof(double), h->stream));
    for (size_t si = 0; si < h->sets.size(); si++)
        if ((rc = reset_marker_set(h, (int)si, h->sets[si]))) return rc;
    if (h->mm.nfixcol > 0) {
        HCHK(hipMemsetAsync(h->mm.d_bfix, 0, (size_t)h->mm.nfixcol * sizeof(double), h->stream));
        HCHK(hipMemsetAsync(h->mm.d_sum_bfix, 0, (size_t)h->mm.nfixcol * sizeof(double), h->stream));
    }
    for (auto &R : h->mm.rnd) {  // u = 0, varU = its prior value (src/mme.jl:200, 265-272), empty sums
        const size_t qk = (size_t)R.q * (size_t)R.tk;
        std::vector<double> vu(2 * R.varU0M.size(), 0.0);
        std::copy(R.varU0M.begin(), R.varU0M.end(), vu.begin());
        HCHK(hipMemsetAsync(R.d_u, 0, qk * sizeof(double), h->stream));
        HCHK(hipMemsetAsync(R.d_sum_u, 0, qk * sizeof(double), h->stream));
        HCHK(hipMemcpyAsync(R.d_vu, vu.data(), vu.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HCHK(hipStreamSynchronize(h->stream));
        R.fine_calls = 0;
    }
    for (auto &V : h->mm.lv) {  // BayesLV sets: zeta back to its start, c = 0, varZeta its prior value, empty sums (src/mme.jl:429-437)
        int rc2 = lv_reset(h, V);
        if (rc2) return rc2;
    }
    for (auto &Rc : h->mm.rc) {  // BayesRCpi sets: annotProb = annot / its row sum, no category yet, empty sums (src/mme.jl:393-399)
        int rc2 = rc_reset(h, Rc);
        if (rc2) return rc2;
    }
    HCHK(hipStreamSynchronize(h->stream));
    h->iter = 0; h->have_y = true; h->poisoned = false; h->ntrace = 0;
    for (auto &hs : h->sets) hs.fine_calls = 0;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_residual_prior(ngp_handle *h, double df, double scale) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(std::isfinite(df) && std::isfinite(scale) && df > 0 && scale >= 0, NGP_ERR_ARG, "bad residual prior");
    h->e_df = df; h->e_scale = scale;
    return NGP_OK;
    NGP_CATCH(h)
}
// weighted residuals (E.str == "D", src/mme.jl:71-75): kept on the host until the panel is set, which scales its rows by sqrt(w)
int32_t ngp_set_residual_weights(ngp_handle *h, const double *w, int64_t N) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->pm, NGP_ERR_STATE,
            "residual weights must be set before the panel (they scale its rows) and before ngp_set_y");
    if (w == nullptr && N == 0) { h->h_rw.clear(); h->sum_w = 0.0; return NGP_OK; }
    REQUIRE(w != nullptr && N > 0, NGP_ERR_ARG, "residual weights: N > 0 entries (or NULL and 0 to remove them)");
    REQUIRE(h->req.storage == NGP_STORAGE_F32, NGP_ERR_ARG,
            "residual weights with compact storage (NGP_STORAGE_U8) are not supported: the byte tiles centre analytically and cannot carry row scales");
    double sw = 0.0;
    for (int64_t i = 0; i < N; i++) {
        REQUIRE(std::isfinite(w[i]) && w[i] > 0.0, NGP_ERR_ARG, "residual weights must be finite and > 0 (w_i = 1 / d_ii)");
        sw = sw + w[i];  // sum_w: index order, left to right (the intercept's lhs, k_head)
    }
    h->h_rw.assign(w, w + N);
    h->sum_w = sw;
    return NGP_OK;
    NGP_CATCH(h)
}
int32_t ngp_get_residual_weights(ngp_handle *h, double *w, int64_t N) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->h_rw.empty(), NGP_ERR_STATE, "no residual weights set on this handle");
    REQUIRE(w != nullptr && N == (int64_t)h->h_rw.size(), NGP_ERR_ARG, "residual weights buffer must hold N entries");
    std::copy(h->h_rw.begin(), h->h_rw.end(), w);
    return NGP_OK;
    NGP_CATCH(h)
}
int32_t ngp_set_intercept(ngp_handle *h, int32_t on) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    h->intercept = on ? 1 : 0;
    return NGP_OK;
    NGP_CATCH(h)
}
int32_t ngp_set_schedule(ngp_handle *h, int64_t chainLength, int64_t burnIn, int64_t thin) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(chainLength >= 0 && burnIn >= 0 && thin >= 1, NGP_ERR_ARG, "bad schedule");
    h->chainLength = chainLength; h->burnIn = burnIn; h->thin = thin;
    return NGP_OK;
    NGP_CATCH(h)
}

}  // extern "C"

namespace {
// checks and trace buffers in front of a run of niter iterations
int prepare_run(ngp_handle *h, int64_t niter) {
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = ready(h))) return rc;
    REQUIRE(niter >= 0, NGP_ERR_ARG, "niter must be >= 0");
    REQUIRE(!h->poisoned, NGP_ERR_STATE, "an earlier sweep was abandoned half-way: set the state again (ngp_set_y / ngp_set_state)");
    REQUIRE(h->mm.ntvb <= h->nvb, NGP_ERR_STATE, "more variance traces requested than the model has variance components");
    if (h->mm.ntl + h->mm.ntvb + (int64_t)h->sets.size() > 0 && h->mm.d_trace_loci && niter > h->mm.trace_ext_cap) {
        if ((rc = h->mm.d_tr_beta.alloc(h, (size_t)niter * std::max<int64_t>(h->mm.ntl, 1)))) return rc;
        if ((rc = h->mm.d_tr_vb.alloc(h, (size_t)niter * std::max<int64_t>(h->mm.ntvb, 1)))) return rc;
        if ((rc = h->mm.d_tr_pi.alloc(h, (size_t)niter * std::max<size_t>(h->sets.size(), 1)))) return rc;
        h->mm.trace_ext_cap = niter;
    }
    if (niter > h->hm.trace_cap) {
        if ((rc = h->hm.d_tr_varE.alloc(h, (size_t)niter))) return rc;
        if ((rc = h->hm.d_tr_b.alloc(h, (size_t)niter))) return rc;
        h->hm.trace_cap = niter;
    }
    h->ntrace = niter;
    if ((rc = ensure_genvar(h, false))) return rc;
    if ((rc = ensure_diag(h, false))) return rc;
    return ensure_prediction(h, false);
}

// K chains per pass over the panel (k_sweep_multi, ngp_sweep.h): can these handles' chains share ONE sweep launch?  They must
// share one panel (ngp_share_panel) and run the engine the fused kernel is built for: persistent sweep, fp32 tiles, phase streamer
// on shards of at most 64 rows, lag 6 or 8, no diagnostics -- and the fused grid must fit the device.  Any marker method may sit in
// any chain: a BayesRCpi set anywhere in the pass selects k_sweep_multi_rc (pick_kernel), on the same three streamer families.

bool fusable(ngp_handle **hs, int n) {
    if (n < 2 || n > NGP_MAXC) return false;
    ngp_handle *h0 = hs[0];
    if (!h0->pm || h0->plan.mode != 1 || h0->plan.V != 1) return false;
    const bool phase = h0->req.storage == 0 && h0->plan.streamer == 1 && h0->plan.R <= 64 && (h0->plan.D == 6 || h0->plan.D == 8);   // role_streamer_multi
    const bool rows = h0->req.storage == 0 && h0->plan.streamer == 2 && (h0->plan.D >= 4 && h0->plan.D <= 6) && n == 2 &&        // role_streamer_rows_multi
                      streamer_lds(h0->plan, n) <= NGP_LDS_MAX;
    bool bytes = false;                                                                                     // ... over byte tiles
    if (h0->req.storage == 1 && h0->plan.streamer == 3 && n <= 3 && streamer_lds(h0->plan, n) <= NGP_LDS_MAX) {
        const int nt = ngp_u8_tasks((int)h0->plan.R);  // update tasks per lane: what the delay line leaves for more chains' arithmetic
        bytes = (nt == 1 && (h0->plan.D == 4 || h0->plan.D == 6 || h0->plan.D == 8)) || (nt == 2 && (h0->plan.D == 4 || h0->plan.D == 8)) || (nt == 4 && n == 2 && h0->plan.D == 4);
    }
    if (!phase && !rows && !bytes) return false;
    bool rcset = false;
    for (int i = 0; i < n; i++) {
        ngp_handle *h = hs[i];
        if (h->pm != h0->pm || h->device != h0->device || h->dbg_mode != 0 || h->hm.d_dbg || h->dbg_census_fail_iter > 0) return false;
        rcset = rcset || !h->mm.rc.empty();
    }
    // a BayesRCpi set in any chain: k_sweep_multi_rc, whose samplers stage the Tuple coefficients beside their own
    if (rcset && sweep_lds(h0->plan, SweepKernel::multi_rc, n) > NGP_LDS_MAX) return false;
    // (the samplers sit at blocks 0, 8, .., 8 (n - 1) of the grid -- one XCD under round-robin placement: the grid must reach the last)
    const int64_t grid = sweep_grid(h0->plan, n);
    return grid <= h0->cu_count && grid > (int64_t)8 * (n - 1);
}

// niter iterations of n chains, every iteration ONE fused sweep launch on the first handle's stream; each chain's small kernels
// (head, coefficients, variance draws, posterior sums) run there too, chain after chain.  Bit for bit what each chain draws alone.
int run_fused(ngp_handle **hs, int n, int64_t niter) {
    ngp_handle *h = hs[0];  // errors are reported on the leader (and copied to the others by the caller)
    int rc;
    for (int i = 0; i < n; i++)
        if ((rc = prepare_run(hs[i], niter))) { if (i) h->err = hs[i]->err; return rc; }
    bool tup = false, rset = false, rcset = false;  // a chain with a Tuple / BayesR / BayesRCpi set: the fused kernel whose samplers hold that chain
    for (int i = 0; i < n; i++) { tup = tup || hs[i]->ntuple > 0; rset = rset || hs[i]->nclass_total > 0; rcset = rcset || !hs[i]->mm.rc.empty(); }
    const SweepKernel kern = pick_kernel(h->plan, n, false, tup, rset, rcset);
    const int64_t grid = sweep_grid(h->plan, n);
    const size_t lds = sweep_lds(h->plan, kern, n);
    REQUIRE(lds <= NGP_LDS_MAX, NGP_ERR_STATE, "fused sweep: LDS of a streamer with this many chains exceeds 160 KiB");
    HCHK(hipFuncSetAttribute(sweep_kernel(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // One abort word: the leader's.  The sweep runs on the leader's stream; every chain's small kernels (head, coefficients, variance
    // draws, posterior sums: six launches of a few microseconds each) stay on the chain's OWN stream, tied to the sweep by events --
    // the K chains' small kernels then run side by side instead of one chain after the other (eight chains: 0.34 ms of a 4.35-ms pass).
    struct Events {  // evp[i]: chain i's coefficients are in (i >= 1); evs: the sweep is done.  Destroyed however the call ends.
        std::vector<hipEvent_t> evp;
        hipEvent_t evs = nullptr;
        ~Events() {
            for (hipEvent_t x : evp) if (x) (void)hipEventDestroy(x);
            if (evs) (void)hipEventDestroy(evs);
        }
    } ev;
    ev.evp.assign((size_t)n, nullptr);
    for (int i = 0; i < n; i++) HCHK(hipStreamSynchronize(hs[i]->stream));
    // Every chain's launches read the leader's word through their d_abort view.  The guard only puts each view back to the
    // handle's own word when the call ends, an exception on the way included; it frees nothing (each word stays owned by its
    // handle's abort_mem).
    struct AbortViews {
        ngp_handle **hs;
        int n;
        ~AbortViews() { for (int i = 0; i < n; i++) hs[i]->cm.d_abort = hs[i]->cm.abort_mem; }
    } views{hs, n};
    for (int i = 1; i < n; i++) hs[i]->cm.d_abort = h->cm.d_abort;
    hipError_t e = hipSuccess;
    for (int i = 1; i < n && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ev.evp[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev.evs, hipEventDisableTiming);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("fused run: ") + hipGetErrorString(e));
    auto sync_all = [&]() {
        hipError_t r = hipStreamSynchronize(h->stream);
        for (int i = 1; i < n; i++) { hipError_t q = hipStreamSynchronize(hs[i]->stream); if (r == hipSuccess) r = q; }
        return r;
    };
    // prediction: ONE pass over the prediction panel per kept iteration serves every chain of the call whose marker sets lie on the same
    // columns as the leader's; a chain with another layout launches its own
    std::vector<char> pred_with_leader((size_t)n, 0);
    for (int i = 0; i < n; i++) pred_with_leader[(size_t)i] = predicts(hs[i]) && same_pred_items(h, hs[i]);
    // genomic variance: the same -- one pass per kept iteration for every chain whose sets AND windows equal the leader's
    std::vector<char> gv_with_leader((size_t)n, 0);
    for (int i = 0; i < n; i++) gv_with_leader[(size_t)i] = gv_active(h) && gv_active(hs[i]) && same_genvar(h, hs[i]);
    CuLease lease(h, grid);
    e = hipEventRecord(h->ev0, h->stream);
    rc = NGP_OK;
    for (int64_t it = 0; it < niter && rc == NGP_OK && e == hipSuccess; ++it) {
        MultiArgs M;
        M.K = n; M.pair = fused_pair(h->plan, n);
        for (int i = 0; i < n; i++) {
            iteration_pre(hs[i], it, false);
            fill_sweep_args(hs[i], 0, hs[i]->NBLK, M.a[i]);
            if (i > 0) {  // the sweep waits for this chain's coefficients (and cleared hand-off counters)
                (void)hipEventRecord(ev.evp[i], hs[i]->stream);
                (void)hipStreamWaitEvent(h->stream, ev.evp[i], 0);
            }
        }
        for (int i = 1; i < n; i++) { M.a[i].census = nullptr; M.a[i].xcc_w = M.a[0].xcc_w; }
        launch_sweep_kernel(kern, grid, lds, h->stream, &M);
        h->sweep_launches += 1; h->last_grid = grid;
        (void)hipEventRecord(ev.evs, h->stream);
        for (int i = 1; i < n; i++) (void)hipStreamWaitEvent(hs[i]->stream, ev.evs, 0);
        for (int i = 0; i < n && rc == NGP_OK; i++) { rc = iteration_post(hs[i], it, !pred_with_leader[(size_t)i], !gv_with_leader[(size_t)i]); if (rc && i) h->err = hs[i]->err; }
        if (rc) break;
        {   // the chains kept in this iteration, served together on the leader's stream (their effects are final: the sweep ran there)
            ngp_handle *served[NGP_PRED_MAXK];
            int ns = 0;
            for (int i = 0; i < n; i++)
                if (pred_with_leader[(size_t)i] && is_kept(hs[i], hs[i]->iter)) served[ns++] = hs[i];
            if (ns > 0) launch_predict(h, served, ns);
            ns = 0;
            for (int i = 0; i < n; i++)
                if (gv_with_leader[(size_t)i] && is_kept(hs[i], hs[i]->iter)) served[ns++] = hs[i];
            if (ns > 0) {  // the pass reads each chain's effects and varE: the chain's next iteration waits for it
                rc = launch_genvar(h, served, ns);
                (void)hipEventRecord(ev.evs, h->stream);
                for (int i = 0; i < ns; i++)
                    if (served[i] != h) (void)hipStreamWaitEvent(served[i]->stream, ev.evs, 0);
            }
        }
        if ((it & 15) == 15 || it + 1 == niter) {  // bound the launch queue
            e = sync_all();
            if (e == hipSuccess) {
                rc = check_abort(h);  // (no retry: there is one grid, and the lease covers it)
                if (rc) for (int i = 1; i < n; i++) { hs[i]->poisoned = true; hs[i]->err = h->err; }
            }
        }
    }
    if (e == hipSuccess) e = sync_all();
    else (void)sync_all();
    if (e == hipSuccess) e = hipEventRecord(h->ev1, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("fused run: ") + hipGetErrorString(e));
    if (rc) return rc;
    float ms = 0.f;
    HCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    for (int i = 0; i < n; i++) { hs[i]->iter_ms += ms; hs[i]->iters_timed += niter; }
    for (int i = 0; i < n; i++)
        if ((rc = sample_flush(hs[i]))) { if (i) h->err = hs[i]->err; return rc; }
    return NGP_OK;
}
}  // namespace

extern "C" {

int32_t ngp_run(ngp_handle *h, int64_t niter) {
    NGP_TRY
    int rc;
    if ((rc = prepare_run(h, niter))) return rc;
    CuLease lease(h);
    HCHK(hipEventRecord(h->ev0, h->stream));
    if ((rc = run_iterations(h, niter, lease, nullptr))) return rc;
    HCHK(hipEventRecord(h->ev1, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    float ms = 0.f;
    HCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->iter_ms += ms; h->iters_timed += niter;
    if ((rc = sample_flush(h))) return rc;
    if (h->dbg_mode != 0) return fail(h, NGP_ERR_DEBUG, "diagnostic timing mode " + std::to_string(h->dbg_mode) + " is active: the chain is invalid (ngp_debug_set_mode(h, 0) ends it)");
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_state(ngp_handle *h, double *ycorr, double *beta, int64_t *delta, double *varBeta, double *piHat, double *varE,
                      double *b, int64_t *iter) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && h->have_y, NGP_ERR_STATE, "panel / y not set");
    HCHK(hipStreamSynchronize(h->stream));
    if (ycorr && h->cm.d_rs) {  // weighted residuals: ycorr = y~ / s
        DevArray<double> d_t;
        if ((rc = d_t.alloc(h, (size_t)h->N))) return rc;
        launch_rows(h, d_t, h->cm.d_ycorr, true);
        hipError_t e = hipMemcpyAsync(ycorr, d_t, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("get_state: ") + hipGetErrorString(e));
    } else if (ycorr) HCHK(hipMemcpy(ycorr, h->cm.d_ycorr, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost));
    if (beta) HCHK(hipMemcpy(beta, h->cm.d_beta, (size_t)h->P * sizeof(double), hipMemcpyDeviceToHost));
    if (delta) {
        std::vector<uint8_t> d((size_t)h->P);
        HCHK(hipMemcpy(d.data(), h->cm.d_delta, (size_t)h->P, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < h->P; k++) delta[k] = d[k];
    }
    if (varBeta && h->nvb) HCHK(hipMemcpy(varBeta, h->mm.d_varBeta, (size_t)h->nvb * sizeof(double), hipMemcpyDeviceToHost));
    if (piHat && !h->sets.empty()) {
        std::vector<DSet> ds(h->sets.size());
        HCHK(hipMemcpy(ds.data(), h->cm.d_sets, ds.size() * sizeof(DSet), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < ds.size(); s++) { piHat[2 * s] = ds[s].piHat0; piHat[2 * s + 1] = ds[s].piHat1; }
    }
    DScal sc;
    HCHK(hipMemcpy(&sc, h->cm.d_scal, sizeof(DScal), hipMemcpyDeviceToHost));
    if (varE) *varE = sc.varE;
    if (b) *b = sc.b;
    if (iter) *iter = h->iter;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_state(ngp_handle *h, const double *ycorr, const double *beta, const int64_t *delta, const double *varBeta,
                      const double *piHat, double varE, double b, int64_t iter) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && h->have_y, NGP_ERR_STATE, "panel / y not set");
    // (varE is 0 before the first iteration -- ngp_set_y -- and drawn before it is used; any later state has varE > 0)
    REQUIRE(std::isfinite(varE) && (varE > 0.0 || (varE == 0.0 && iter == 0)) && std::isfinite(b) && iter >= 0, NGP_ERR_ARG,
            "bad scalar state (varE must be finite and positive)");
    if (ycorr) HCHK(hipMemcpy(h->cm.d_ycorr, ycorr, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice));
    if (ycorr && h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, false);  // weighted residuals: y~ = s ycorr
    if (beta) HCHK(hipMemcpy(h->cm.d_beta, beta, (size_t)h->P * sizeof(double), hipMemcpyHostToDevice));
    if (delta) {
        std::vector<uint8_t> d((size_t)h->P);
        for (int64_t k = 0; k < h->P; k++) d[k] = (uint8_t)(delta[k] != 0);
        HCHK(hipMemcpy(h->cm.d_delta, d.data(), (size_t)h->P, hipMemcpyHostToDevice));
    }
    if (varBeta && h->nvb) HCHK(hipMemcpy(h->mm.d_varBeta, varBeta, (size_t)h->nvb * sizeof(double), hipMemcpyHostToDevice));
    if (piHat)
        for (size_t s = 0; s < h->sets.size(); s++)
            hipLaunchKernelGGL(k_set_pi, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, (int)s, piHat[2 * s], piHat[2 * s + 1]);
    DScal sc;
    HCHK(hipMemcpy(&sc, h->cm.d_scal, sizeof(DScal), hipMemcpyDeviceToHost));
    sc.varE = varE; sc.iVarE = 1.0 / varE; sc.b = b;
    HCHK(hipMemcpy(h->cm.d_scal, &sc, sizeof(DScal), hipMemcpyHostToDevice));
    HCHK(hipStreamSynchronize(h->stream));
    h->iter = iter;
    if (ycorr && beta) h->poisoned = false;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_trace(ngp_handle *h, double *varE, double *b, int64_t n) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    n = std::min(n, h->ntrace);
    if (n <= 0) return NGP_OK;
    if (varE) HCHK(hipMemcpy(varE, h->hm.d_tr_varE, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (b) HCHK(hipMemcpy(b, h->hm.d_tr_b, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_posterior_sums(ngp_handle *h, double *sum_beta, double *sum_beta2, double *sum_delta, double *sum_varBeta,
                               double *sum_pi, double *sum_varE, double *sum_b, int64_t *nKept) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    HCHK(hipStreamSynchronize(h->stream));
    const size_t pb = (size_t)h->P * sizeof(double);
    if (sum_beta) HCHK(hipMemcpy(sum_beta, h->cm.d_sum_beta, pb, hipMemcpyDeviceToHost));
    if (sum_beta2) HCHK(hipMemcpy(sum_beta2, h->cm.d_sum_beta2, pb, hipMemcpyDeviceToHost));
    if (sum_delta) HCHK(hipMemcpy(sum_delta, h->cm.d_sum_delta, pb, hipMemcpyDeviceToHost));
    if (sum_varBeta && h->nvb) HCHK(hipMemcpy(sum_varBeta, h->mm.d_sum_varBeta, (size_t)h->nvb * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_pi && !h->sets.empty()) {
        std::vector<DSet> ds(h->sets.size());
        HCHK(hipMemcpy(ds.data(), h->cm.d_sets, ds.size() * sizeof(DSet), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < ds.size(); s++) { sum_pi[2 * s] = ds[s].sum_pi0; sum_pi[2 * s + 1] = ds[s].sum_pi1; }
    }
    DScal sc;
    HCHK(hipMemcpy(&sc, h->cm.d_scal, sizeof(DScal), hipMemcpyDeviceToHost));
    if (sum_varE) *sum_varE = sc.sum_varE;
    if (sum_b) *sum_b = sc.sum_b;
    if (nKept) *nKept = sc.nKept;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_posterior_len(ngp_handle *h, int64_t *len) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(len != nullptr, NGP_ERR_ARG, "null len");
    *len = posterior_words(h);
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_export_posterior_device(ngp_handle *h, void *device_ptr, int64_t len) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    ChainState st;
    describe(h, st);
    const Plan pl = place(st, posterior_layout);
    REQUIRE(device_ptr && len == (int64_t)(pl.bytes / 8), NGP_ERR_ARG, "export buffer length mismatch (see ngp_posterior_len)");
    if ((rc = stage(h, st))) return rc;
    HCHK(copy_segments(pl, device_ptr, false, true, h->stream));
    return NGP_OK;
    NGP_CATCH(h)
}

namespace {
// one fine-seam call; dev: the caller's arrays (and piHat) are DEVICE memory of this handle's device, delta is int64 there too
int sweep_set_impl(ngp_handle *h, int32_t set_id, double varE, double *ycorr, double *beta, int64_t *delta, double *varBeta, double *piHat, bool dev) {
    int rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->records_only, NGP_ERR_STATE, "this handle has records but no genotype panel (ngp_set_records): it takes no marker sets and sweeps none");
    REQUIRE(set_id >= 0 && set_id < (int)h->sets.size(), NGP_ERR_ARG, "unknown set id");
    REQUIRE(ycorr && beta && varBeta, NGP_ERR_ARG, "null state pointer");
    REQUIRE(std::isfinite(varE) && varE > 0.0, NGP_ERR_ARG, "varE must be finite and positive");
    if ((rc = sync_tables(h))) return rc;
    if ((rc = sync_linear_blocks(h, (int)set_id))) return rc;
    HSet &hs = h->sets[set_id];
    const int64_t nvbs = (int64_t)hs.vb0.size();  // variance entries of the set: regions (loci for BayesB), k x k per region for a tuple set
    // (device arrays are not read back to be looked at: a variance that is not finite poisons the chain visibly -- k_prep -- as in ngp_run)
    if (!dev) for (int64_t r = 0; r < nvbs; r++) REQUIRE(std::isfinite(varBeta[r]) && (varBeta[r] >= 0.0 || hs.tk > 1), NGP_ERR_ARG, "varBeta must be finite, >= 0");
    const bool has_pi = hs.method != NGP_METHOD_BAYESPR && hs.method != NGP_METHOD_TUPLE && hs.method != NGP_METHOD_BAYESLV && hs.method != NGP_METHOD_BAYESRC;
    if (has_pi) REQUIRE(piHat != nullptr, NGP_ERR_ARG, "BayesB / BayesC need piHat");
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const uint64_t it = ++hs.fine_calls;
    const int64_t tb0 = hs.col0 / NGP_BLK, tb1 = (hs.col0 + hs.ncol - 1) / NGP_BLK + 1;
    CuLease lease(h);
    for (int attempt = 0;; ++attempt) {
        HCHK(hipMemsetAsync(h->cm.d_ycorr, 0, (size_t)h->L * sizeof(double), h->stream));
        HCHK(hipMemcpyAsync(h->cm.d_ycorr, ycorr, (size_t)h->N * sizeof(double), in, h->stream));
        if (h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, false);  // weighted residuals: the caller's ycorr into y~ = s ycorr
        HCHK(hipMemcpyAsync(h->cm.d_beta + hs.col0, beta, (size_t)hs.ncol * sizeof(double), in, h->stream));
        HCHK(hipMemcpyAsync(h->mm.d_varBeta + hs.vb_off, varBeta, (size_t)nvbs * sizeof(double), in, h->stream));
        if (has_pi) {
            if (dev) hipLaunchKernelGGL(k_set_pi_dev, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, (int)set_id, (const double *)piHat);
            else hipLaunchKernelGGL(k_set_pi, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, (int)set_id, piHat[0], piHat[1]);
        }
        hipLaunchKernelGGL(k_set_varE, dim3(1), dim3(1), 0, h->stream, h->cm.d_scal, varE);
        // (no draws, no intercept: ycorr'ycorr of the caller's residual sets the scale of the fixed-point accumulators)
        hipLaunchKernelGGL(k_head, dim3(1), dim3(1024), 0, h->stream, h->cm.d_ycorr, (long long)h->L, (long long)h->N, h->cm.d_scal, h->e_df,
                           h->e_scale, 0, 0, h->seed, (uint64_t)h->chain, it, (double *)nullptr, (double *)nullptr, (long long)0, h->cm.d_abort, h->pm->mpm_max,
                           (const double *)h->cm.d_rs, h->sum_w);
        hipLaunchKernelGGL(k_prep, dim3((unsigned)(h->Ppad / 256 + 1)), dim3(256), 0, h->stream, (long long)h->Ppad, h->cm.d_setof, h->cm.d_loc,
                           h->cm.d_vbidx, h->cm.d_sets, h->cm.d_scal, h->mm.d_varBeta, h->pm->mpm, h->cm.d_lhs0, h->cm.d_rhs0, h->cm.d_beta, h->cm.d_c, h->cm.d_w,
                           h->cm.d_q, h->cm.d_T, h->cm.d_chi, (int)set_id, h->seed, (uint64_t)h->chain, it, (long long)h->h_regs.size(), h->mm.d_regs, h->mm.d_regchi, h->mm.d_rcls,
                           h->cm.d_ccnt, (long long)(h->plan.mode == 1 ? h->cm.ccnt_words : 0), h->cm.d_abort, h->mm.d_tup, h->mm.d_tupc, h->mm.d_tupg, (const DRc *)h->mm.d_rctab.get());
        launch_tinv(h);
        launch_sweep(h, tb0, tb1, nullptr);
        launch_variance(h, (int)set_id, it);
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipGetLastError());
        int64_t itf = 0;
        rc = check_abort(h, &itf);
        if (rc == NGP_RETRY_CENSUS && attempt == 0) {  // nothing was changed (the caller's arrays are the state): once more, alone on the device
            h->exclusive = true; h->census_retries += 1;
            lease.make_exclusive();
            continue;
        }
        if (rc) return rc;
        break;
    }
    if (h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, true);  // ... and back: the caller's ycorr is unscaled (d_ycorr is scratch here)
    HCHK(hipMemcpyAsync(ycorr, h->cm.d_ycorr, (size_t)h->N * sizeof(double), out, h->stream));
    HCHK(hipMemcpyAsync(beta, h->cm.d_beta + hs.col0, (size_t)hs.ncol * sizeof(double), out, h->stream));
    HCHK(hipMemcpyAsync(varBeta, h->mm.d_varBeta + hs.vb_off, (size_t)nvbs * sizeof(double), out, h->stream));
    if (dev) {
        if (delta) hipLaunchKernelGGL(k_delta_widen, dim3((unsigned)((hs.ncol + 255) / 256)), dim3(256), 0, h->stream, (const uint8_t *)(h->cm.d_delta + hs.col0), (long long *)delta, (long long)hs.ncol);
        if (piHat) hipLaunchKernelGGL(k_get_pi_dev, dim3(1), dim3(1), 0, h->stream, (const DSet *)h->cm.d_sets, (int)set_id, piHat);
    }
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    if (h->dbg_mode != 0) return fail(h, NGP_ERR_DEBUG, "diagnostic timing mode is active: the sweep is invalid");
    if (dev) return NGP_OK;
    if (delta) {
        std::vector<uint8_t> d((size_t)hs.ncol);
        HCHK(hipMemcpy(d.data(), h->cm.d_delta + hs.col0, (size_t)hs.ncol, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < hs.ncol; k++) delta[k] = d[k];
    }
    if (piHat) {
        DSet ds;
        HCHK(hipMemcpy(&ds, h->cm.d_sets + set_id, sizeof(DSet), hipMemcpyDeviceToHost));
        piHat[0] = ds.piHat0; piHat[1] = ds.piHat1;
    }
    return NGP_OK;
}
}  // namespace

int32_t ngp_sweep_set(ngp_handle *h, int32_t set_id, double varE, double *ycorr, double *beta, int64_t *delta, double *varBeta,
                      double *piHat) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    return sweep_set_impl(h, set_id, varE, ycorr, beta, delta, varBeta, piHat, false);
    NGP_CATCH(h)
}

/* The fine seam with the caller's state in DEVICE memory (a host that keeps ycorr, beta, varBeta on the GPU between the calls of
 * src/samplers.jl:52 -- ROCArrays -- pays no PCIe round trip per set and iteration): device-to-device copies on the handle's stream. */
int32_t ngp_sweep_set_dev(ngp_handle *h, int32_t set_id, double varE, void *d_ycorr, void *d_beta, void *d_delta, void *d_varBeta, void *d_piHat) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    return sweep_set_impl(h, set_id, varE, (double *)d_ycorr, (double *)d_beta, (int64_t *)d_delta, (double *)d_varBeta, (double *)d_piHat, true);
    NGP_CATCH(h)
}

int32_t ngp_get_timing(ngp_handle *h, int64_t *sweep_launches, double *iter_ms, int64_t *iters) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (sweep_launches) *sweep_launches = h->sweep_launches;
    if (iter_ms) *iter_ms = h->iter_ms;
    if (iters) *iters = h->iters_timed;
    h->sweep_launches = 0; h->iter_ms = 0; h->iters_timed = 0;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_profile_iteration(ngp_handle *h, double *avg_ms, int64_t *launches, double *bytes_per_launch) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->records_only, NGP_ERR_STATE, "this handle has records but no genotype panel (ngp_set_records): it takes no marker sets and sweeps none");
    if ((rc = ready(h))) return rc;
    const int64_t n = (h->plan.mode == 1) ? 1 : h->NBLK;
    std::vector<hipEvent_t> evs((size_t)(2 * n));
    for (auto &e : evs) HCHK(hipEventCreate(&e));
    if (h->hm.trace_cap < 1) {
        if ((rc = h->hm.d_tr_varE.alloc(h, 1))) return rc;
        if ((rc = h->hm.d_tr_b.alloc(h, 1))) return rc;
        h->hm.trace_cap = 1;
    }
    h->ntrace = 1;
    CuLease lease(h);
    rc = run_iterations(h, 1, lease, evs.data());  // (checks the abort word; a launch that ends at its census is run again)
    hipError_t e = hipStreamSynchronize(h->stream);
    double tot = 0.0;
    if (rc == NGP_OK && e == hipSuccess)
        for (int64_t i = 0; i < n; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, evs[2 * i], evs[2 * i + 1]);
            tot += ms;
        }
    for (auto &ev : evs) (void)hipEventDestroy(ev);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("profile_iteration: ") + hipGetErrorString(e));
    if (avg_ms) *avg_ms = tot / (double)n;
    if (launches) *launches = n;
    const double bpe = (h->req.storage == 1) ? 1.0 : 4.0;  // algorithmic bytes per genotype: the panel is read once per iteration
    if (bytes_per_launch) *bytes_per_launch = (h->plan.mode == 1) ? (double)h->N * (double)h->P * bpe : (double)h->N * NGP_BLK * bpe;
    return rc;
    NGP_CATCH(h)
}

int32_t ngp_debug_stamps(ngp_handle *h, int32_t enable, uint64_t *out, int64_t n) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const size_t words = (size_t)2 << 20;
    REQUIRE(!(enable && !h->mm.rc.empty()), NGP_ERR_ARG, "time stamps exist in the diagnostic kernel only, which does not carry the rule of BayesRCpi sets");
    if (enable && !h->hm.d_dbg) { if ((rc = h->hm.d_dbg.alloc(h, words))) return rc; HCHK(hipStreamSynchronize(h->stream)); }
    if (out && h->hm.d_dbg) HCHK(hipMemcpy(out, h->hm.d_dbg, std::min<size_t>((size_t)n, words) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (!enable && h->hm.d_dbg) { HCHK(hipStreamSynchronize(h->stream)); h->hm.d_dbg.reset(); }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_configure(ngp_handle *h, int32_t mode, int32_t lag) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->pm, NGP_ERR_STATE, "ngp_configure must precede the panel upload");
    REQUIRE(mode == 0 || mode == 1, NGP_ERR_ARG, "mode must be 0 (per-block launches) or 1 (persistent sweep)");
    REQUIRE(lag >= 1 && lag <= NGP_MAX_LAG, NGP_ERR_ARG, "lag must be in 1..12 (above 8: compact storage)");
    h->req.mode = mode; h->req.lag = lag; h->req.lag_auto = false;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_near_lags(ngp_handle *h, int32_t near) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->pm, NGP_ERR_STATE, "ngp_set_near_lags must precede the panel upload");
    REQUIRE(near >= 0 && near <= 4, NGP_ERR_ARG, "near lags: 0 (automatic) or 1..4");
    h->req.near_req = near;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_near_lags(ngp_handle *h, int32_t *near) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (near) *near = h->plan.near;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_chain_form(ngp_handle *h, int32_t form) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(form == 0 || form == 1, NGP_ERR_ARG, "chain form: 0 (64 steps per block) or 1 (linear blocks by the inverse form)");
    // the table of linear blocks and its flags belong to the form they were built under.  (Belt and braces: sync_linear_blocks already
    // drops the key whenever it clears the flags, which alone keeps "flags zero behind a matching key" impossible.)
    if (form != h->chain_form) h->cm.blin_for = -2;
    h->chain_form = form;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_chain_form(ngp_handle *h, int32_t *form) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (form) *form = h->chain_form;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_config(ngp_handle *h, int32_t *mode, int32_t *lag) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (mode) *mode = h->req.mode;  // (after the panel: the engine in force, see alloc_panel)
    if (lag) *lag = h->plan.D;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_draws_indexed(ngp_handle *h, uint64_t iter, uint64_t kind, uint64_t index0, int32_t what, double p1, double p2, int64_t n,
                          double *out) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(out && n > 0, NGP_ERR_ARG, "bad output buffer");
    DevArray<double> d;
    if ((rc = d.alloc(h, (size_t)n))) return rc;
    hipLaunchKernelGGL(k_draws_indexed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->seed, (uint64_t)h->chain, iter, kind,
                       index0, what, p1, p2, (long long)n, d);
    hipError_t e = hipMemcpyAsync(out, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("draws: ") + hipGetErrorString(e));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_eval_math(ngp_handle *h, int32_t which, const double *in, int64_t n, double *out) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(in && out && n > 0, NGP_ERR_ARG, "bad buffers");
    DevArray<double> di, dout;
    if ((rc = di.alloc(h, (size_t)n))) return rc;
    if ((rc = dout.alloc(h, (size_t)n))) return rc;
    hipError_t e = hipMemcpyAsync(di, in, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream);
    hipLaunchKernelGGL(k_eval_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, which, di, (long long)n, dout);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("eval_math: ") + hipGetErrorString(e));
    return NGP_OK;
    NGP_CATCH(h)
}


/* ------------------------------------------------------------------------------------------------
 * round 2 additions: diagnostics out of the environment, posterior-sum restore, snapshots, traces,
 * streamer variants, pooled posterior sums
 * ---------------------------------------------------------------------------------------------- */
int32_t ngp_debug_set_mode(ngp_handle *h, int32_t mode) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(mode >= 0 && mode <= 6, NGP_ERR_ARG, "diagnostic mode must be in 0..6");
    REQUIRE(mode == 0 || h->mm.rc.empty(), NGP_ERR_ARG, "timing modes exist in the diagnostic kernel only, which does not carry the rule of BayesRCpi sets");
    h->dbg_mode = mode;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_debug_set_knob(ngp_handle *h, int32_t knob) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    h->knob = knob;
    h->gram_engine = (knob & 1024) ? 1 : 0;  // bit 10: build the Gram window on the matrix cores instead of the fp64 VALU kernel (same bits)
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_streamer(ngp_handle *h, int32_t variant) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->pm, NGP_ERR_STATE, "ngp_set_streamer must precede the panel upload");
    REQUIRE((variant >= 0 && variant <= 2) || variant == 4 || variant == 6, NGP_ERR_ARG,
            "streamer variant: 0 (automatic), 1 (phase streamer), 2 (row-owning waves) or 4 / 6 (row-owning waves, two / three shards per workgroup)");
    h->req.streamer_req = variant;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_max_shards(ngp_handle *h, int32_t max_shards) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->pm, NGP_ERR_STATE, "ngp_set_max_shards must precede the panel upload");
    REQUIRE(max_shards >= 0, NGP_ERR_ARG, "max_shards: 0 (automatic) or a positive number of streamer workgroups");
    h->req.max_shards_req = max_shards;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_shards_for_chains(ngp_handle *h, int32_t chains, int32_t *max_shards) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(chains >= 1 && max_shards, NGP_ERR_ARG, "chains must be >= 1");
    // workgroups go to the 8 XCDs in turn: `chains` grids are co-resident when each takes at most (CUs / 8) / chains CUs per XCD;
    // a grid is 1 sampler + ceil(S / 32) reducers + S streamers
    const int per = 8 * ((h->cu_count / 8) / chains);
    const int s = per - 1 - (per + NGP_GRP - 1) / NGP_GRP;
    REQUIRE(s >= 1, NGP_ERR_ARG, "too many chains for this device");
    *max_shards = s;
    return NGP_OK;
    NGP_CATCH(h)
}

/* K chains per pass, set-up: h takes `owner`'s panel (tiles, Gram window, x'x, column means) by reference -- no copy, no second
 * 120 GB -- together with its engine, layout and storage; everything that belongs to a chain (effects, residuals, variances, draws,
 * hand-off rings, posterior sums) is h's own.  The arrays live as long as any handle refers to them. */
int32_t ngp_share_panel(ngp_handle *h, ngp_handle *owner) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(owner && owner != h && owner->pm, NGP_ERR_ARG, "ngp_share_panel: the owner has no panel");
    REQUIRE(owner->device == h->device, NGP_ERR_ARG, "ngp_share_panel: both handles must be on one device");
    REQUIRE(!owner->panel_open, NGP_ERR_STATE, "ngp_share_panel: the owner's panel is still open (ngp_end_panel)");
    HCHK(hipStreamSynchronize(owner->stream));
    h->cu_count = owner->cu_count;
    if ((rc = alloc_panel(h, owner->N, owner->P, owner))) return rc;
    h->records_only = owner->records_only;
    return NGP_OK;
    NGP_CATCH(h)
}

/* The largest max_shards (ngp_set_max_shards, before the panel is set) with which `chains` chains share ONE fused sweep launch:
 * chains x (1 sampler + ceil(S / 32) reducers) + S streamers <= CUs. */
int32_t ngp_shards_for_pass(ngp_handle *h, int32_t chains, int32_t *max_shards) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(chains >= 1 && chains <= NGP_MAXC && max_shards, NGP_ERR_ARG, "chains per pass: 1..8");
    SweepPlan p;  // (the phase streamer, one shard per workgroup: the engine this serves)
    int s = h->cu_count;
    for (; s >= 1; --s) {
        p.S = s; p.NG = (s + NGP_GRP - 1) / NGP_GRP;
        if (sweep_grid(p, chains) <= h->cu_count) break;
    }
    REQUIRE(s >= 1, NGP_ERR_ARG, "too many chains for this device");
    *max_shards = s;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_storage(ngp_handle *h, int32_t storage) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(!h->pm, NGP_ERR_STATE, "ngp_set_storage must precede the panel upload");
    REQUIRE(storage == NGP_STORAGE_F32 || storage == NGP_STORAGE_U8, NGP_ERR_ARG, "storage: 0 (fp32 tiles) or 1 (compact: bytes + column means)");
    REQUIRE(storage == NGP_STORAGE_F32 || h->h_rw.empty(), NGP_ERR_ARG,
            "residual weights with compact storage (NGP_STORAGE_U8) are not supported: the byte tiles centre analytically and cannot carry row scales");
    h->req.storage = storage;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_storage(ngp_handle *h, int32_t *storage, double *means, int64_t P) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (storage) *storage = h->req.storage;
    if (means) {
        REQUIRE(h->pm, NGP_ERR_STATE, "column means exist after the panel is set");
        REQUIRE(P == h->P, NGP_ERR_ARG, "means buffer must hold P entries");
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipMemcpy(means, h->pm->mean, (size_t)P * sizeof(double), hipMemcpyDeviceToHost));
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_streamer(ngp_handle *h, int32_t *variant, int32_t *gemv_chains) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (variant) *variant = (h->req.mode == 1) ? h->plan.streamer : 0;
    if (gemv_chains) *gemv_chains = h->plan.nchain;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_posterior_sums(ngp_handle *h, const double *sum_beta, const double *sum_beta2, const double *sum_delta,
                               const double *sum_varBeta, const double *sum_pi, double sum_varE, double sum_b, int64_t nKept) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && h->have_y, NGP_ERR_STATE, "panel / y not set");
    REQUIRE(sum_beta && sum_beta2 && sum_delta && nKept >= 0 && std::isfinite(sum_varE) && std::isfinite(sum_b), NGP_ERR_ARG, "bad posterior sums");
    REQUIRE(h->nvb == 0 || sum_varBeta, NGP_ERR_ARG, "sum_varBeta missing");
    REQUIRE(h->sets.empty() || sum_pi, NGP_ERR_ARG, "sum_pi missing");
    HCHK(hipStreamSynchronize(h->stream));
    const size_t pb = (size_t)h->P * sizeof(double);
    HCHK(hipMemcpy(h->cm.d_sum_beta, sum_beta, pb, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(h->cm.d_sum_beta2, sum_beta2, pb, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(h->cm.d_sum_delta, sum_delta, pb, hipMemcpyHostToDevice));
    if (h->nvb) HCHK(hipMemcpy(h->mm.d_sum_varBeta, sum_varBeta, (size_t)h->nvb * sizeof(double), hipMemcpyHostToDevice));
    for (size_t si = 0; si < h->sets.size(); si++)
        hipLaunchKernelGGL(k_set_sum_pi, dim3(1), dim3(1), 0, h->stream, h->cm.d_sets, (int)si, sum_pi[2 * si], sum_pi[2 * si + 1]);
    HCHK(hipStreamSynchronize(h->stream));
    DScal sc;
    HCHK(hipMemcpy(&sc, h->cm.d_scal, sizeof(DScal), hipMemcpyDeviceToHost));
    sc.sum_varE = sum_varE; sc.sum_b = sum_b; sc.nKept = nKept;
    HCHK(hipMemcpy(h->cm.d_scal, &sc, sizeof(DScal), hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Snapshot file: the chain state and the posterior sums (the byte sequence: ngp_state.h).  It plays the role of the reference's
 * append-only *Out files for a resumed run (src/outFiles.jl:17-21): what was kept before the interruption is not lost. */
namespace {
// the model a snapshot belongs to (equal counts are not enough), in the words of the file.  An unweighted chain without
// random-effect sets writes neither flag, digest nor random part: its bytes are those of the first snapshots.
struct ModelSig {
    std::vector<int64_t> sets;  // per marker set {method, K + 16 tuple k + the BayesLV word, nreg, col0, ncol}
    int64_t nfs = 0;            // fixed-effect sets | NGP_SNAP_WEIGHTED | NGP_SNAP_RANDOM | NGP_SNAP_HOLDOUT | NGP_SNAP_LIABILITY | NGP_SNAP_FIXVARE
    uint64_t digest = 0;        // of the residual weights
    uint64_t ho_digest = 0;     // of the held-out rows
    uint64_t lb_digest = 0;     // of the augmented rows and their classes or bounds
    double fix_varE = 0.0;      // the fixed residual variance
    std::vector<uint64_t> rnd;  // nrand | per set q, digest of its level coding and K
    std::vector<int64_t> fix;   // ncol per fixed-effect set
    ModelSig() = default;
    explicit ModelSig(const ngp_handle *h) {
        for (auto &hs : h->sets) sets.insert(sets.end(), {hs.method, hs.K + 16 * hs.tk + lv_sig(h, hs) + rc_sig(h, hs), hs.nreg, hs.col0, hs.ncol});
        nfs = (int64_t)h->mm.fix.size() | (h->h_rw.empty() ? 0 : NGP_SNAP_WEIGHTED) | (h->mm.rnd.empty() ? 0 : NGP_SNAP_RANDOM) |
              (h->cm.ho_rows.empty() ? 0 : NGP_SNAP_HOLDOUT) | (h->cm.lb.on() ? NGP_SNAP_LIABILITY : 0) | (h->fix_varE > 0.0 ? NGP_SNAP_FIXVARE : 0);
        lb_digest = liab_sig_digest(h->cm.lb.digest, h->cm.lb.ts_mode, (bool)h->cm.lb.d_sum_prob); fix_varE = h->fix_varE;
        if (!h->h_rw.empty()) digest = weights_digest(h->h_rw);
        if (!h->cm.ho_rows.empty()) ho_digest = rows_digest(h->cm.ho_rows);
        if (!h->mm.rnd.empty()) {
            rnd.push_back((uint64_t)h->mm.rnd.size());
            for (auto &R : h->mm.rnd) { rnd.push_back((uint64_t)rand_q_word(R)); rnd.push_back(R.sig); }
        }
        for (auto &fx : h->mm.fix) fix.push_back(fx.ncol);
    }
};
// delta of a snapshot is 0 / 1 (a BayesR set's classes are drawn anew by the next sweep)
void snapshot_delta_01(const Plan &body, std::vector<unsigned char> &img) {
    unsigned char *d = img.data() + body.off(SEG_DELTA);
    for (size_t k = 0; k < body.size(SEG_DELTA); k++) d[k] = (unsigned char)(d[k] != 0);
}
}  // namespace

int32_t ngp_save_snapshot(ngp_handle *h, const char *path) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && h->have_y, NGP_ERR_STATE, "panel / y not set");
    REQUIRE(path != nullptr, NGP_ERR_ARG, "null path");
    REQUIRE(!h->poisoned, NGP_ERR_STATE, "the chain state is invalid (abandoned sweep)");
    ChainState st;
    describe(h, st);
    if ((rc = stage(h, st))) return rc;
    const Plan head = place(st, snapshot_head_layout), body = place(st, snapshot_body_layout);
    std::vector<unsigned char> himg(head.bytes), img(body.bytes);
    HCHK(copy_segments(head, himg.data(), true, true, h->stream));
    HCHK(copy_segments(body, img.data(), true, true, h->stream));
    snapshot_delta_01(body, img);
    const ModelSig sig(h);
    const std::string tmp = std::string(path) + ".tmp";
    File f(fopen(tmp.c_str(), "wb"));
    if (!f) return fail(h, NGP_ERR_ARG, "cannot open " + tmp + " for writing");
    bool ok = true;
    auto W = [&](const void *p, size_t n) { if (n && fwrite(p, 1, n, f.get()) != n) ok = false; };
    const int64_t dims[4] = {h->N, h->P, h->nvb, (int64_t)h->sets.size()};
    W("NGPSNAP2", 8); W(dims, sizeof(dims)); W(himg.data(), himg.size());
    W(sig.sets.data(), sig.sets.size() * 8); W(&sig.nfs, 8);
    if (sig.nfs & NGP_SNAP_WEIGHTED) W(&sig.digest, 8);
    if (sig.nfs & NGP_SNAP_HOLDOUT) W(&sig.ho_digest, 8);
    if (sig.nfs & NGP_SNAP_LIABILITY) W(&sig.lb_digest, 8);
    if (sig.nfs & NGP_SNAP_FIXVARE) W(&sig.fix_varE, 8);
    W(sig.rnd.data(), sig.rnd.size() * 8); W(sig.fix.data(), sig.fix.size() * 8);
    W(img.data(), img.size());
    if (fclose(f.release()) != 0) ok = false;  // (a failed close is a failed write)
    if (!ok || rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); return fail(h, NGP_ERR_ARG, std::string("writing the snapshot failed: ") + path); }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_load_snapshot(ngp_handle *h, const char *path) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && h->have_y, NGP_ERR_STATE, "panel / y not set (build the model first, then load the snapshot)");
    REQUIRE(path != nullptr, NGP_ERR_ARG, "null path");
    File f(fopen(path, "rb"));
    if (!f) return fail(h, NGP_ERR_ARG, std::string("cannot open snapshot ") + path);
    ChainState st;
    describe(h, st);
    if ((rc = stage(h, st))) return rc;
    const Plan head = place(st, snapshot_head_layout), body = place(st, snapshot_body_layout);
    std::vector<unsigned char> himg(head.bytes), img(body.bytes);
    bool ok = true;
    auto Rd = [&](void *p, size_t n) { if (n && fread(p, 1, n, f.get()) != n) ok = false; };
    auto word = [](const std::vector<unsigned char> &im, size_t off) { int64_t v; memcpy(&v, im.data() + off, 8); return v; };
    auto real = [](const std::vector<unsigned char> &im, size_t off) { double v; memcpy(&v, im.data() + off, 8); return v; };
    char magic[8]; int64_t dims[4] = {0, 0, 0, 0};
    Rd(magic, 8); Rd(dims, sizeof(dims)); Rd(himg.data(), himg.size());
    if (!ok || memcmp(magic, "NGPSNAP2", 8) != 0) return fail(h, NGP_ERR_ARG, "not a snapshot file (bad magic or truncated header)");
    const int64_t iter = word(himg, head.off(SEG_ITER));
    if (dims[0] != h->N || dims[1] != h->P || dims[2] != h->nvb || dims[3] != (int64_t)h->sets.size() || iter < 0 || word(himg, head.off(SEG_NKEPT)) < 0)
        return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (N, P, variance components or marker sets differ)");
    {   // model signature: the file's against this handle's
        const ModelSig want(h);
        ModelSig got;
        got.sets.assign(want.sets.size(), -1); got.nfs = -1;
        Rd(got.sets.data(), got.sets.size() * 8); Rd(&got.nfs, 8);
        const bool snap_w = ok && got.nfs >= 0 && (got.nfs & NGP_SNAP_WEIGHTED) != 0, snap_r = ok && got.nfs >= 0 && (got.nfs & NGP_SNAP_RANDOM) != 0;
        const bool snap_h = ok && got.nfs >= 0 && (got.nfs & NGP_SNAP_HOLDOUT) != 0;
        if (snap_w) Rd(&got.digest, 8);
        if (snap_h) Rd(&got.ho_digest, 8);
        const bool snap_l = ok && got.nfs >= 0 && (got.nfs & NGP_SNAP_LIABILITY) != 0, snap_f = ok && got.nfs >= 0 && (got.nfs & NGP_SNAP_FIXVARE) != 0;
        if (snap_l) Rd(&got.lb_digest, 8);
        if (snap_f) Rd(&got.fix_varE, 8);
        if (ok && snap_l != h->cm.lb.on())
            return fail(h, NGP_ERR_ARG, snap_l ? "snapshot of a chain with liability traits: this handle has none (ngp_set_liability_classes / ngp_set_liability_bounds)"
                                               : "snapshot of a chain without liability traits: this handle has them");
        if (ok && snap_l && got.lb_digest != want.lb_digest) {
            const Liab &lb = h->cm.lb;
            const bool prob = (bool)lb.d_sum_prob;
            for (int w = 0; w < 4; w++) {  // the same rows and classes under another threshold step, or with / without class probabilities?
                if (got.lb_digest != liab_sig_digest(lb.digest, w & 1, (w & 2) != 0)) continue;
                if ((w & 1) != lb.ts_mode)
                    return fail(h, NGP_ERR_ARG, (w & 1) ? "snapshot of a chain under Cowles' threshold step: this handle runs Albert-Chib (ngp_set_threshold_step)"
                                                        : "snapshot of a chain under the Albert-Chib threshold step: this handle runs Cowles' (ngp_set_threshold_step)");
                return fail(h, NGP_ERR_ARG, prob ? "snapshot of a chain without class probabilities: this handle has them (ngp_enable_class_probabilities)"
                                                 : "snapshot of a chain with class probabilities: this handle has none (ngp_enable_class_probabilities)");
            }
            return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (its liability rows, classes or bounds differ)");
        }
        if (ok && (snap_f != (h->fix_varE > 0.0) || (snap_f && got.fix_varE != want.fix_varE)))
            return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (its residual variance is fixed at another value, or sampled)");
        if (ok && snap_h != !h->cm.ho_rows.empty())
            return fail(h, NGP_ERR_ARG, snap_h ? "snapshot of a chain with held-out records: this handle has none (ngp_set_holdout)"
                                               : "snapshot of a chain without held-out records: this handle has them");
        if (ok && snap_h && got.ho_digest != want.ho_digest)
            return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (its held-out records differ)");
        if (ok && snap_r != !want.rnd.empty())
            return fail(h, NGP_ERR_ARG, snap_r ? "snapshot of a chain with random-effect sets: this handle has none (ngp_add_random_set)"
                                               : "snapshot of a chain without random-effect sets: this handle has them");
        if (snap_r) {
            got.rnd.assign(want.rnd.size(), 0);
            Rd(got.rnd.data(), got.rnd.size() * 8);
            if (!ok || got.rnd != want.rnd)
                return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (its random-effect sets differ: levels, level coding or K)");
        }
        if (ok && snap_w != !h->h_rw.empty())
            return fail(h, NGP_ERR_ARG, snap_w ? "snapshot of a chain with residual weights: this handle has none (ngp_set_residual_weights)"
                                               : "snapshot of a chain without residual weights: this handle has them");
        if (ok && snap_w && got.digest != want.digest)
            return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (its residual weights differ)");
        bool same = ok && got.sets == want.sets && got.nfs == want.nfs;
        if (same) { got.fix.assign(want.fix.size(), -1); Rd(got.fix.data(), got.fix.size() * 8); same = got.fix == want.fix; }
        if (!ok) return fail(h, NGP_ERR_ARG, "snapshot file is truncated (model signature)");
        if (!same)
            return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (methods, classes, regions or fixed-effect sets differ)");
    }
    const size_t have = fread(img.data(), 1, img.size(), f.get());
    const double varE = real(img, body.off(SEG_VARE));
    if (have >= body.off(SEG_VARE) + 8 && !(std::isfinite(varE) && (varE > 0.0 || (varE == 0.0 && iter == 0))))
        return fail(h, NGP_ERR_ARG, "snapshot holds an invalid residual variance");
    if (have >= body.off(SEG_NFIX) + 8 && word(img, body.off(SEG_NFIX)) != h->mm.nfixcol)
        return fail(h, NGP_ERR_ARG, "snapshot does not match the model of this handle (fixed-effect columns differ)");
    char extra;
    if (have != img.size() || fread(&extra, 1, 1, f.get()) != 0) return fail(h, NGP_ERR_ARG, "snapshot file is truncated or has trailing bytes");
    REQUIRE(std::isfinite(real(img, body.off(SEG_B))), NGP_ERR_ARG, "bad scalar state (varE must be finite and positive)");
    REQUIRE(std::isfinite(real(img, body.off(SEG_SUM_VARE))) && std::isfinite(real(img, body.off(SEG_SUM_B))), NGP_ERR_ARG, "bad posterior sums");
    snapshot_delta_01(body, img);
    h->poisoned = true;  // until the whole restore has gone through: a failure half-way must not leave a mixed state behind as valid
    HCHK(copy_segments(head, himg.data(), true, false, h->stream));
    HCHK(copy_segments(body, img.data(), true, false, h->stream));
    if ((rc = commit(h, st, true, true))) return rc;
    h->chain = (uint32_t)st.chain64;  // (with the seed: the draws continue the interrupted chain's streams)
    h->poisoned = false;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_trace_loci(ngp_handle *h, const int64_t *loci, int64_t n, int64_t n_varBeta) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(n >= 0 && n <= 4096 && (n == 0 || loci) && n_varBeta >= 0, NGP_ERR_ARG, "at most 4096 traced loci");
    for (int64_t i = 0; i < n; i++) REQUIRE(loci[i] >= 0 && loci[i] < h->P, NGP_ERR_ARG, "traced locus outside the panel");
    HCHK(hipStreamSynchronize(h->stream));
    h->mm.d_trace_loci.reset(); h->mm.d_tr_beta.reset(); h->mm.d_tr_vb.reset(); h->mm.d_tr_pi.reset();
    h->mm.trace_ext_cap = 0; h->mm.ntl = n; h->mm.ntvb = n_varBeta;
    if (n == 0 && n_varBeta == 0) return NGP_OK;
    if ((rc = h->mm.d_trace_loci.alloc(h, (size_t)std::max<int64_t>(n, 1)))) return rc;
    if (n) HCHK(hipMemcpy(h->mm.d_trace_loci, loci, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_trace_ext(ngp_handle *h, double *beta_tr, double *varBeta_tr, double *pi_tr, int64_t n) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->mm.d_trace_loci != nullptr, NGP_ERR_STATE, "no traces requested (ngp_set_trace_loci)");
    n = std::min(n, std::min(h->ntrace, h->mm.trace_ext_cap));
    if (n <= 0) return NGP_OK;
    HCHK(hipStreamSynchronize(h->stream));
    const int64_t ntvb = std::min<int64_t>(h->mm.ntvb, h->nvb);
    REQUIRE(ntvb == h->mm.ntvb, NGP_ERR_STATE, "more variance traces requested than the model has variance components");
    if (beta_tr && h->mm.ntl) HCHK(hipMemcpy(beta_tr, h->mm.d_tr_beta, (size_t)(n * h->mm.ntl) * sizeof(double), hipMemcpyDeviceToHost));
    if (varBeta_tr && h->mm.ntvb) HCHK(hipMemcpy(varBeta_tr, h->mm.d_tr_vb, (size_t)(n * h->mm.ntvb) * sizeof(double), hipMemcpyDeviceToHost));
    if (pi_tr && !h->sets.empty()) HCHK(hipMemcpy(pi_tr, h->mm.d_tr_pi, (size_t)n * h->sets.size() * sizeof(double), hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}


/* Pooled posterior sums of n independent chains (one handle each): afterwards every handle holds the sums over all chains
 * (nKept included), so posterior means come from any of them.  Handles on DIFFERENT devices are reduced by ONE RCCL
 * all-reduce (ncclSum, fp64) over xGMI -- RCCL is loaded on first use (dlopen), the library has no link-time dependency on
 * it; handles that SHARE a device are added on that device first.  Single-process form of the end-of-run exchange
 * (SURVEY.md section 8 e); bench.py's multi-process form uses torch.distributed on the same packed buffer. */
namespace {
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *nm : names) { lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
        if (!lib) { err = std::string("cannot load RCCL: ") + (dlerror() ? dlerror() : "?"); return false; }
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        AllReduce = (decltype(AllReduce))dlsym(lib, "ncclAllReduce");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!CommInitAll || !AllReduce || !GroupStart || !GroupEnd || !CommDestroy) { err = "RCCL symbols missing"; dlclose(lib); lib = nullptr; return false; }
        return true;
    }
} g_rccl;

int import_posterior_device(ngp_handle *h, const double *o) {  // inverse of ngp_export_posterior_device
    ChainState st;
    describe(h, st);
    int rc;
    if ((rc = stage(h, st))) return rc;
    HCHK(copy_segments(place(st, posterior_layout), const_cast<double *>(o), false, false, h->stream));
    st.sc.nKept = (long long)std::llround(st.nkept_f64);
    return commit(h, st, false, true);
}
}  // namespace

int32_t ngp_run_many(ngp_handle **hs, int32_t n, int64_t niter) {
    NGP_TRY
    if (!hs || n < 1) return fail(nullptr, NGP_ERR_ARG, "ngp_run_many: no handles");
    for (int i = 0; i < n; i++) {
        if (!hs[i]) return fail(nullptr, NGP_ERR_ARG, "ngp_run_many: null handle");
        for (int k = 0; k < i; k++)
            if (hs[k] == hs[i]) return fail(hs[0], NGP_ERR_ARG, "ngp_run_many: the same handle twice");
        if (hs[i]->cm.lb.on() != hs[0]->cm.lb.on() || hs[i]->cm.lb.C != hs[0]->cm.lb.C)  // one trait per call: liabilities on every chain or on none
            return fail(hs[0], NGP_ERR_ARG, "ngp_run_many: the chains of a call all carry liability traits of one kind (classes, bounds) or none does");
    }
    // chains that share one panel (ngp_share_panel) and run the engine the fused kernel serves take ONE sweep launch per iteration:
    // the panel is streamed once for all of them (K chains per pass)
    if (fusable(hs, n)) return run_fused(hs, n, niter);
    // one host thread per chain, as a caller would do it (src/samplers.jl:23: one chain per Julia task); the chains of a device run
    // side by side when their grids fit it together (ngp_set_max_shards), in turns otherwise (CuLease)
    std::vector<int32_t> rcs((size_t)n, NGP_OK);
    struct Joiner {  // a std::thread constructor that throws (system_error) must not unwind past joinable threads
        std::vector<std::thread> th;
        ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); }
    } jn;
    jn.th.reserve((size_t)n);
    // ngp_run is itself an entry point behind the exception barrier: nothing can leave a worker's lambda
    for (int i = 1; i < n; i++) jn.th.emplace_back([&rcs, hs, niter, i]() noexcept { rcs[(size_t)i] = ngp_run(hs[i], niter); });
    rcs[0] = ngp_run(hs[0], niter);
    for (auto &t : jn.th) t.join();
    for (int i = 0; i < n; i++)
        if (rcs[(size_t)i] != NGP_OK) return rcs[(size_t)i];  // the message is on that handle (ngp_last_error)
    return NGP_OK;
    NGP_CATCH((hs ? hs[0] : nullptr))
}

int32_t ngp_allreduce_posterior(ngp_handle **hs, int32_t n) {
    NGP_TRY
    if (!hs || n < 1) return fail(nullptr, NGP_ERR_ARG, "ngp_allreduce_posterior: no handles");
    for (int i = 0; i < n; i++)
        if (!hs[i]) return fail(nullptr, NGP_ERR_ARG, "ngp_allreduce_posterior: null handle");
    ngp_handle *h = hs[0];  // errors are reported on the first handle
    int rc;
    if ((rc = enter(h))) return rc;
    ChainState st0;
    describe(h, st0);
    const Plan pl0 = place(st0, posterior_layout);
    const int64_t len = (int64_t)(pl0.bytes / 8);
    for (int i = 0; i < n; i++) {
        REQUIRE(hs[i]->pm, NGP_ERR_STATE, "ngp_allreduce_posterior: a handle has no panel");
        ChainState sti;  // one model: the packed posteriors hold the same segments, each of the same length
        describe(hs[i], sti);
        REQUIRE(place(sti, posterior_layout).same_shape(pl0), NGP_ERR_ARG, "ngp_allreduce_posterior: the chains do not share one model");
        // (sum_fit is indexed by the record, sum_prob by the position in the hold-out set: it pools only over chains with one mask)
        REQUIRE(!hs[i]->cm.lb.d_sum_prob || hs[i]->cm.ho_rows == h->cm.ho_rows, NGP_ERR_ARG,
                "ngp_allreduce_posterior: class probabilities are summed by position in the hold-out set and these chains hold out different records "
                "(pool fold-chains on the host, from ngp_get_class_probabilities)");
        for (int k = 0; k < i; k++) REQUIRE(hs[k] != hs[i], NGP_ERR_ARG, "ngp_allreduce_posterior: a handle is listed twice");
    }
    struct Buffers {  // the packed sums of every handle, on its device: freed there, with that device current
        ngp_handle **hs;
        std::vector<DevArray<double>> b;
        ~Buffers() {
            for (size_t i = 0; i < b.size(); i++)
                if (b[i]) { (void)hipSetDevice(hs[i]->device); b[i].reset(); }
        }
    } bufs{hs, std::vector<DevArray<double>>((size_t)n)};
    std::vector<DevArray<double>> &buf = bufs.b;
    for (int i = 0; i < n; i++) {
        if ((rc = enter(hs[i]))) return rc;
        if (buf[i].alloc_raw((size_t)len) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "posterior buffer");
        if ((rc = ngp_export_posterior_device(hs[i], buf[i], len))) { if (hs[i] != h) h->err = hs[i]->err; return rc; }
    }
    // leaders: the first handle of every device; the others are added into their leader on the device
    auto devof = [](const ngp_handle *x) { return x->vdev >= 0 ? 1000 + x->vdev : x->device; };  // (virtual devices: test hook)
    std::vector<int> leader((size_t)n);
    std::vector<int> leaders;
    for (int i = 0; i < n; i++) {
        leader[i] = i;
        for (int k = 0; k < i; k++) if (devof(hs[k]) == devof(hs[i])) { leader[i] = leader[k]; break; }
        if (leader[i] == i) leaders.push_back(i);
    }
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; i++)
        if (leader[i] != i) {
            ngp_handle *L = hs[leader[i]];
            (void)hipSetDevice(L->device);
            hipLaunchKernelGGL(k_add_inplace, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, L->stream, buf[leader[i]], buf[i], (long long)len);
            e = hipStreamSynchronize(L->stream);
        }
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("pooling on one device: ") + hipGetErrorString(e));
    if (leaders.size() > 1) {
        const int nl = (int)leaders.size();
        bool one_physical = true;
        for (int i = 1; i < nl; i++) one_physical = one_physical && hs[leaders[i]]->device == hs[leaders[0]]->device;
        if (one_physical) {
            // every leader on one GPU (virtual devices, ngp_debug_set_virtual_device): the collective is a sum on that GPU, leader
            // order -- the same packing, grouping and unpacking as across devices, everything but the ncclAllReduce call
            ngp_handle *L0 = hs[leaders[0]];
            (void)hipSetDevice(L0->device);
            DevArray<double> tot;  // (freed at the end of this block, L0's device current)
            if (tot.alloc_raw((size_t)len) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "posterior buffer");
            e = hipMemcpyAsync(tot, buf[leaders[0]], (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, L0->stream);
            for (int i = 1; i < nl && e == hipSuccess; i++)
                hipLaunchKernelGGL(k_add_inplace, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, L0->stream, tot, buf[leaders[i]], (long long)len);
            for (int i = 0; i < nl && e == hipSuccess; i++)
                e = hipMemcpyAsync(buf[leaders[i]], tot, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, L0->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(L0->stream);
            if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("pooling leaders on one device: ") + hipGetErrorString(e));
        } else {
        if (!g_rccl.load()) return fail(h, NGP_ERR_HIP, g_rccl.err);
        std::vector<void *> comms((size_t)nl, nullptr);
        std::vector<int> devs((size_t)nl);
        for (int i = 0; i < nl; i++) devs[i] = hs[leaders[i]]->device;
        int r = g_rccl.CommInitAll(comms.data(), nl, devs.data());
        if (r == 0) {
            g_rccl.GroupStart();
            for (int i = 0; i < nl && r == 0; i++) {
                ngp_handle *L = hs[leaders[i]];
                (void)hipSetDevice(L->device);
                r = g_rccl.AllReduce(buf[leaders[i]], buf[leaders[i]], (size_t)len, /*ncclDouble*/ 8, /*ncclSum*/ 0, comms[i], L->stream);
            }
            const int r2 = g_rccl.GroupEnd();
            if (r == 0) r = r2;
            for (int i = 0; i < nl; i++) { (void)hipSetDevice(devs[i]); (void)hipStreamSynchronize(hs[leaders[i]]->stream); }
        }
        for (int i = 0; i < nl; i++) if (comms[i]) g_rccl.CommDestroy(comms[i]);
        if (r != 0) return fail(h, NGP_ERR_HIP, std::string("RCCL all-reduce failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?"));
        }
    }
    for (int i = 0; i < n; i++) {
        (void)hipSetDevice(hs[i]->device);
        if ((rc = import_posterior_device(hs[i], buf[leader[i]]))) { if (hs[i] != h) h->err = hs[i]->err; return rc; }
    }
    return NGP_OK;
    NGP_CATCH((hs ? hs[0] : nullptr))
}


/* BayesR marker set (src/runTime.jl:78-93, set-up src/mme.jl:374-383, sampler src/functions.jl:238-289): ONE variance for the set
 * (varBeta0), K <= 4 variance classes with multipliers vClass[v] of that variance (a class with multiplier 0 = effect exactly
 * 0) and class probabilities pi[v]; estPi: pi ~ Dirichlet(nLoci + 1) after every sweep.  delta holds the class of a locus,
 * counted from 1 as the reference writes it. */
int32_t ngp_add_marker_set_r(ngp_handle *h, int64_t col0, int64_t ncol, double df, double scale, double varBeta0, const double *vClass,
                             const double *pi, int32_t K, int32_t estPi, const double *lhs0, const double *rhs0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = check_marker_slot(h, col0, ncol, ncol, "marker set outside the panel"))) return rc;
    REQUIRE(vClass && pi && K >= 2 && K <= NGP_RMAX, NGP_ERR_ARG, "BayesR needs 2..16 variance classes with their probabilities");
    if ((rc = check_classes(h, "BayesR", vClass, pi, K))) return rc;
    REQUIRE(std::isfinite(varBeta0) && varBeta0 > 0.0, NGP_ERR_ARG, "BayesR varBeta0 must be positive");
    REQUIRE(std::isfinite(df) && std::isfinite(scale) && df > 0, NGP_ERR_ARG, "df/scale must be finite, df > 0");
    MarkerSetSpec sp;
    sp.hs = HSet{col0, ncol, NGP_METHOD_BAYESR, df, scale, 1, h->nvb, estPi, 0, 0.5, std::vector<double>(1, varBeta0)};
    sp.hs.K = K; sp.hs.vcls.assign(vClass, vClass + K); sp.hs.rpi.assign(pi, pi + K);
    sp.ds = dset(NGP_METHOD_BAYESR, estPi, df, scale, col0, ncol);
    sp.ds.K = K;
    for (int v = 0; v < K; v++) sp.ds.vcls[v] = vClass[v];
    column_loci(sp, h->nvb, 0);  // one variance for the set, one region: drawn with BayesPR's regions
    const int64_t rs = 0, re = ncol;
    sp.regions = MarkerSetSpec::sumsq; sp.reg_start = &rs; sp.reg_stop = &re;
    sp.lhs0 = lhs0; sp.rhs0 = rhs0;
    return commit_marker_set(h, sp, set_id);
    NGP_CATCH(h)
}

/* BayesRCpi marker set -- annotation-informed BayesR (src/runTime.jl, BayesRCπ(pi, class, v, annot); set-up src/mme.jl:384-403, :493-516;
 * sampler src/functions.jl:291-360): A annotations (columns of annot, entries 0 / 1, column-major with leading dimension ld), K variance
 * classes, one variance per annotation (all start at varBeta0), piHat[a] = pi for every annotation.  1 <= A <= 8, K >= 2, A K <= 16.
 * Refused: a locus without an annotation (the reference divides 0 / 0 there and throws in Categorical: such loci belong in another
 * set), entries other than 0 / 1.  delta holds the class, annotCat the annotation of a locus, both from 1.  Models with such a set
 * run the persistent sweep in kernels of their own (k_sweep_rc; k_sweep_tall_rc on fp32 panels so tall that a streamer workgroup owns
 * several shards; k_sweep_multi_rc for K chains per pass) or the per-block engine. */
int32_t ngp_add_marker_set_rc(ngp_handle *h, int64_t col0, int64_t ncol, double df, double scale, double varBeta0, const double *vClass,
                              const double *pi, int32_t K, const int32_t *annot, int64_t ld, int32_t A, int32_t estPi, const double *lhs0,
                              const double *rhs0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = check_marker_slot(h, col0, ncol, ncol, "marker set outside the panel"))) return rc;
    REQUIRE(vClass && pi && annot, NGP_ERR_ARG, "BayesRCpi: classes, their probabilities or the annotations missing");
    REQUIRE(K >= 2 && A >= 1 && A <= NGP_AMAX && (int64_t)A * K <= NGP_RMAX, NGP_ERR_ARG,
            "BayesRCpi needs K >= 2 classes and 1..8 annotations with A * K <= 16");
    REQUIRE(ld >= ncol, NGP_ERR_ARG, "BayesRCpi: leading dimension of annot smaller than ncol");
    REQUIRE(std::isfinite(df) && std::isfinite(scale) && df > 0, NGP_ERR_ARG, "df/scale must be finite, df > 0");
    REQUIRE(!h->hm.d_dbg && h->dbg_mode == 0, NGP_ERR_ARG, "BayesRCpi sets run in a kernel without time stamps and timing modes: switch the diagnostics off first");
    if ((rc = check_classes(h, "BayesRCpi", vClass, pi, K))) return rc;
    REQUIRE(std::isfinite(varBeta0) && varBeta0 > 0.0, NGP_ERR_ARG, "BayesRCpi varBeta0 must be positive");
    HRc Rc;
    Rc.set = (int)h->sets.size(); Rc.A = A; Rc.Kc = K; Rc.n = ncol; Rc.nseg = (ncol + NGP_SEG - 1) / NGP_SEG;
    Rc.mask.assign((size_t)ncol, 0);
    for (int64_t l = 0; l < ncol; l++) {
        for (int a = 0; a < A; a++) {
            const int32_t e = annot[(size_t)a * (size_t)ld + (size_t)l];
            REQUIRE(e == 0 || e == 1, NGP_ERR_ARG, "BayesRCpi: annotation entries must be 0 or 1 (locus " + std::to_string(l) + ")");
            if (e) Rc.mask[(size_t)l] |= (uint8_t)(1u << a);
        }
        REQUIRE(Rc.mask[(size_t)l] != 0, NGP_ERR_ARG, "BayesRCpi: locus " + std::to_string(l) + " has no annotation (the reference divides 0 / 0 there, "
                                                      "src/mme.jl:396: such loci belong in another set)");
    }
    const size_t an = (size_t)A * (size_t)ncol;
    if ((rc = Rc.d_mask.alloc(h, (size_t)ncol))) return rc;
    if ((rc = Rc.d_cat.alloc(h, (size_t)ncol))) return rc;
    if ((rc = Rc.d_prob.alloc(h, an))) return rc;
    if ((rc = Rc.d_sum.alloc(h, an))) return rc;
    if ((rc = Rc.d_part.alloc(h, (size_t)Rc.nseg * (size_t)A))) return rc;
    if ((rc = Rc.d_cnt.alloc(h, (size_t)Rc.nseg * NGP_RMAX))) return rc;
    HCHK(hipMemcpy(Rc.d_mask, Rc.mask.data(), (size_t)ncol, hipMemcpyHostToDevice));
    if ((rc = rc_reset(h, Rc))) return rc;
    // the marker set: A variances outside the region tables (k_rc_draw draws them), A * K slots of class state
    const int ns = A * K;
    MarkerSetSpec sp;
    sp.hs = HSet{col0, ncol, NGP_METHOD_BAYESRC, df, scale, (int64_t)A, h->nvb, estPi, 0, 0.5, std::vector<double>((size_t)A, varBeta0)};
    sp.hs.K = ns; sp.hs.rc = (int)h->mm.rc.size();
    sp.ds = dset(NGP_METHOD_BAYESRC, estPi, df, scale, col0, ncol);
    sp.ds.K = ns; sp.ds.rcA = A; sp.ds.rcK = K;
    for (int i = 0; i < ns; i++) {
        sp.hs.vcls.push_back(vClass[i % K]); sp.hs.rpi.push_back(pi[i % K]);
        sp.ds.vcls[i] = vClass[i % K];
    }
    column_loci(sp, h->nvb, 0);  // (the first of the set's A variances: k_prep adds the annotation)
    sp.lhs0 = lhs0; sp.rhs0 = rhs0;
    sp.rc = &Rc;
    return commit_marker_set(h, sp, set_id);
    NGP_CATCH(h)
}

/* The per-locus state of a BayesRCpi set and its class probabilities (any pointer may be null): piHat / sum_pi hold A K entries,
 * annotation-major; annotProb / sum_annot ncol A entries, column-major (locus l, annotation a at l + a ncol); annotCat ncol entries,
 * from 1.  sum_annot[l, a] counts the kept iterations with annotCat[l] = a + 1: divided by the kept iterations it is the
 * posterior membership probability.  The A variances travel with ngp_get_state / ngp_set_state. */
int32_t ngp_get_rc_state(ngp_handle *h, int32_t set_id, double *piHat, double *sum_pi, double *annotProb, int32_t *annotCat, double *sum_annot) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int)h->sets.size() && h->sets[(size_t)set_id].rc >= 0, NGP_ERR_ARG, "not a BayesRCpi set");
    const HSet &hs = h->sets[(size_t)set_id];
    HRc &Rc = h->mm.rc[(size_t)hs.rc];
    HCHK(hipStreamSynchronize(h->stream));
    DSet ds;
    HCHK(hipMemcpy(&ds, h->cm.d_sets + set_id, sizeof(DSet), hipMemcpyDeviceToHost));
    for (int i = 0; i < hs.K; i++) {
        if (piHat) piHat[i] = ds.pic[i];
        if (sum_pi) sum_pi[i] = ds.sum_pic[i];
    }
    const size_t an = (size_t)Rc.A * (size_t)Rc.n;
    if (annotProb) HCHK(hipMemcpy(annotProb, Rc.d_prob, an * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_annot) HCHK(hipMemcpy(sum_annot, Rc.d_sum, an * sizeof(double), hipMemcpyDeviceToHost));
    if (annotCat) {
        std::vector<uint8_t> c8((size_t)Rc.n);
        HCHK(hipMemcpy(c8.data(), Rc.d_cat, (size_t)Rc.n, hipMemcpyDeviceToHost));
        for (int64_t l = 0; l < Rc.n; l++) annotCat[l] = c8[(size_t)l];
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_rc_state(ngp_handle *h, int32_t set_id, const double *piHat, const double *sum_pi, const double *annotProb, const int32_t *annotCat,
                         const double *sum_annot) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int)h->sets.size() && h->sets[(size_t)set_id].rc >= 0, NGP_ERR_ARG, "not a BayesRCpi set");
    const HSet &hs = h->sets[(size_t)set_id];
    HRc &Rc = h->mm.rc[(size_t)hs.rc];
    const size_t an = (size_t)Rc.A * (size_t)Rc.n;
    if (piHat)
        for (int i = 0; i < hs.K; i++) REQUIRE(std::isfinite(piHat[i]) && piHat[i] > 0.0, NGP_ERR_ARG, "BayesRCpi: class probabilities must be > 0");
    if (annotProb)
        for (int64_t l = 0; l < Rc.n; l++)
            for (int a = 0; a < Rc.A; a++) {
                const double p = annotProb[(size_t)a * (size_t)Rc.n + (size_t)l];
                const bool has = (Rc.mask[(size_t)l] >> a) & 1;
                REQUIRE(has ? (std::isfinite(p) && p > 0.0) : p == 0.0, NGP_ERR_ARG,
                        "BayesRCpi: annotProb must be > 0 where the locus has the annotation and 0 elsewhere");
            }
    std::vector<uint8_t> c8;
    if (annotCat) {
        c8.resize((size_t)Rc.n);
        for (int64_t l = 0; l < Rc.n; l++) {
            REQUIRE(annotCat[l] >= 1 && annotCat[l] <= Rc.A, NGP_ERR_ARG, "BayesRCpi: annotCat counts the annotations from 1");
            c8[(size_t)l] = (uint8_t)annotCat[l];
        }
    }
    HCHK(hipStreamSynchronize(h->stream));
    if (piHat || sum_pi)
        if ((rc = set_class_state_dev(h, set_id, hs.K, piHat, sum_pi))) return rc;
    if (annotProb) HCHK(hipMemcpy(Rc.d_prob, annotProb, an * sizeof(double), hipMemcpyHostToDevice));
    if (sum_annot) HCHK(hipMemcpy(Rc.d_sum, sum_annot, an * sizeof(double), hipMemcpyHostToDevice));
    if (annotCat) HCHK(hipMemcpy(Rc.d_cat, c8.data(), (size_t)Rc.n, hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Correlated marker sets -- the Tuple method of BayesPR (src/functions.jl:140-154, sampleVarCovBetaPR :513-516, set-up
 * src/mme.jl:448-489): k sets (breeds) share nloc loci; per locus a k x k conditional, per region an inverse-Wishart draw of the
 * k x k variance matrix.  The panel holds the k columns of a locus side by side: component m of locus l is panel column
 * col0 + 64 (l / Lb) + k (l % Lb) + m with Lb = floor(64 / k) loci per 64-column block and col0 on a block boundary (a locus never
 * straddles two blocks; for k = 3 column 63 of every block of the set is unused: fill it with zeros). */
int32_t ngp_add_marker_set_tuple(ngp_handle *h, int64_t col0, int64_t nloc, int32_t k, double df, const double *scale,
                                 const int64_t *reg_start, const int64_t *reg_stop, int64_t nreg, const double *varBeta0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(k >= 1 && k <= NGP_KMAX, NGP_ERR_ARG, "a tuple holds 1..4 correlated sets");
    REQUIRE(nloc >= 1 && col0 >= 0 && col0 % NGP_BLK == 0, NGP_ERR_ARG, "tuple set: first column on a 64-column block boundary");
    // the set owns its 64-column blocks to the end of the last one (its block chain draws whole loci; no other set's column may sit there)
    const int64_t Lb = NGP_BLK / k, nblk = (nloc + Lb - 1) / Lb, span = NGP_BLK * (nblk - 1) + (int64_t)k * (nloc - Lb * (nblk - 1));
    if ((rc = check_marker_slot(h, col0, span, NGP_BLK * nblk, "tuple set outside the panel"))) return rc;
    REQUIRE(scale && varBeta0 && reg_start && reg_stop && nreg > 0, NGP_ERR_ARG, "scale / varBeta0 / regions missing");
    REQUIRE(std::isfinite(df) && df > 0, NGP_ERR_ARG, "df must be finite and positive");
    REQUIRE((int64_t)nloc * k < ((int64_t)1 << 31), NGP_ERR_ARG, "tuple set too large");
    for (int a = 0; a < k * k; a++) REQUIRE(std::isfinite(scale[a]) && std::isfinite(varBeta0[a]), NGP_ERR_ARG, "scale / varBeta0 must be finite");
    for (int a = 0; a < k; a++) REQUIRE(varBeta0[a * k + a] > 0.0, NGP_ERR_ARG, "varBeta0 must be positive definite");
    if ((rc = check_regions(h, reg_start, reg_stop, nreg, nloc, "regions must cover all loci of the set"))) return rc;
    std::vector<double> vb0((size_t)(nreg * k * k));
    for (int64_t r = 0; r < nreg; r++) for (int a = 0; a < k * k; a++) vb0[(size_t)(r * k * k + a)] = varBeta0[a];  // src/mme.jl:516
    MarkerSetSpec sp;
    sp.hs = HSet{col0, span, NGP_METHOD_TUPLE, df, 0.0, nreg, h->nvb, 0, 0, 0.5, std::move(vb0)};
    sp.hs.tk = k; sp.hs.nloc = nloc;
    sp.ds = dset(NGP_METHOD_TUPLE, 0, df, 0.0, col0, span);
    sp.own0 = col0; sp.own1 = std::min<int64_t>(col0 + NGP_BLK * nblk, h->Ppad);  // (the lanes of the last block behind the last locus: unused)
    for (int64_t r = 0; r < nreg; r++)
        for (int64_t l = reg_start[r]; l < reg_stop[r]; l++)
            for (int m = 0; m < k; m++)  // h_loc is also the key of the component's normal draw
                sp.loci.push_back({tuple_col(col0, k, l, m), (int32_t)(l * k + m), (int32_t)(h->nvb + r * k * k)});
    sp.regions = MarkerSetSpec::tuple; sp.reg_start = reg_start; sp.reg_stop = reg_stop;
    DTup tp;
    memset(&tp, 0, sizeof(tp));
    tp.k = k; tp.col0 = col0; tp.nloc = nloc; tp.vb_off = h->nvb; tp.df = df;
    for (int a = 0; a < k * k; a++) tp.scale[a] = scale[a];
    sp.tup = &tp;
    return commit_marker_set(h, sp, set_id);
    NGP_CATCH(h)
}

int32_t ngp_get_class_state(ngp_handle *h, int32_t set_id, double *piHat, double *sum_pi, int64_t *K) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int)h->sets.size(), NGP_ERR_ARG, "unknown set id");
    HCHK(hipStreamSynchronize(h->stream));
    DSet ds;
    HCHK(hipMemcpy(&ds, h->cm.d_sets + set_id, sizeof(DSet), hipMemcpyDeviceToHost));
    if (K) *K = h->sets[(size_t)set_id].K;
    for (int v = 0; v < h->sets[(size_t)set_id].K; v++) {
        if (piHat) piHat[v] = ds.pic[v];
        if (sum_pi) sum_pi[v] = ds.sum_pic[v];
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_class_state(ngp_handle *h, int32_t set_id, const double *piHat, const double *sum_pi, int64_t K) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int)h->sets.size(), NGP_ERR_ARG, "unknown set id");
    REQUIRE(h->sets[(size_t)set_id].K > 0 && K == h->sets[(size_t)set_id].K, NGP_ERR_ARG, "not a BayesR set, or another number of classes");
    if (piHat) for (int64_t v = 0; v < K; v++) REQUIRE(std::isfinite(piHat[v]) && piHat[v] > 0.0, NGP_ERR_ARG, "class probabilities must be > 0");
    return set_class_state_dev(h, set_id, (int)K, piHat, sum_pi);
    NGP_CATCH(h)
}


/* A fixed-effect set beyond the intercept: the columns of one model term, or of one `blockThese` group (X[xSet].data, N x ncol,
 * column-major; src/prepMatVec.jl:150-165).  Sets are sampled after the intercept in the order they are added -- the order of
 * `keys(X)` at src/samplers.jl:39 (a Julia Dict: the shim passes that order; to put the intercept elsewhere, switch it off and add
 * a column of ones).  One column: sampleX! (src/functions.jl:41-47) with the summary-statistics terms lhs0 / rhs0 (src/mme.jl:140-147);
 * several: sampleb! (src/functions.jl:22-36), Gauss-Seidel over X'X + min|diag| / 10000 (src/mme.jl:149-152). */
int32_t ngp_add_fixed_set(ngp_handle *h, const double *X, int64_t N, int64_t ncol, int64_t ld, const double *lhs0, const double *rhs0,
                          int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open: x'x and the Gram window exist after ngp_end_panel");
    REQUIRE(X && N == h->N && ncol >= 1 && ncol <= 64 && ld >= N, NGP_ERR_ARG, "fixed-effect set: N rows, 1..64 columns");
    REQUIRE(h->mm.fix.size() < 16, NGP_ERR_ARG, "at most 16 fixed-effect sets");
    std::vector<double> xc((size_t)N * ncol), x0((size_t)ncol * ncol), xr;
    for (int64_t a = 0; a < ncol; a++)
        for (int64_t i = 0; i < N; i++) {
            const double v = X[(size_t)a * ld + i];
            REQUIRE(std::isfinite(v), NGP_ERR_ARG, "non-finite value in a fixed-effect column");
            xc[(size_t)a * N + i] = v;
        }
    if (h->cm.d_rs) {  // weighted residuals: the columns of the row-scaled problem, X~ = s X (on the device); X~'X~ below is X'WX
        DevArray<double> d_x;
        if ((rc = d_x.alloc(h, xc.size()))) return rc;
        hipError_t e = hipMemcpyAsync(d_x, xc.data(), xc.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
        for (int64_t a = 0; a < ncol && e == hipSuccess; a++) launch_rows(h, d_x + (size_t)a * N, d_x + (size_t)a * N, false);
        if (e == hipSuccess) e = hipMemcpyAsync(xc.data(), d_x, xc.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("add_fixed_set: ") + hipGetErrorString(e));
    }
    for (int64_t a = 0; a < ncol; a++)
        for (int64_t b = 0; b <= a; b++) {
            double acc = 0.0;
            for (int64_t i = 0; i < N; i++) acc = std::fma(xc[(size_t)a * N + i], xc[(size_t)b * N + i], acc);
            x0[(size_t)a * ncol + b] = acc; x0[(size_t)b * ncol + a] = acc;
        }
    xr = x0;
    if (ncol > 1) {  // src/mme.jl:149-152
        double mn = std::fabs(x0[0]);
        for (int64_t a = 1; a < ncol; a++) mn = std::min(mn, std::fabs(x0[(size_t)a * ncol + a]));
        for (int64_t a = 0; a < ncol; a++) xr[(size_t)a * ncol + a] += mn / 10000.0;
    }
    REQUIRE(x0[0] > 0.0 || ncol > 1, NGP_ERR_ARG, "fixed-effect column is identically zero");
    HFix fx;
    fx.ncol = ncol; fx.off = h->mm.nfixcol;
    std::vector<double> z((size_t)ncol, 0.0);
    if ((rc = fx.d_X.alloc(h, xc.size()))) return rc;
    if ((rc = fx.d_xpx0.alloc(h, x0.size()))) return rc;
    if ((rc = fx.d_xpxR.alloc(h, xr.size()))) return rc;
    if ((rc = fx.d_lhs0.alloc(h, (size_t)ncol))) return rc;
    if ((rc = fx.d_rhs0.alloc(h, (size_t)ncol))) return rc;
    HCHK(hipMemcpy(fx.d_X, xc.data(), xc.size() * sizeof(double), hipMemcpyHostToDevice));
    HCHK(hipMemcpy(fx.d_xpx0, x0.data(), x0.size() * sizeof(double), hipMemcpyHostToDevice));
    HCHK(hipMemcpy(fx.d_xpxR, xr.data(), xr.size() * sizeof(double), hipMemcpyHostToDevice));
    HCHK(hipMemcpy(fx.d_lhs0, lhs0 ? lhs0 : z.data(), (size_t)ncol * sizeof(double), hipMemcpyHostToDevice));
    HCHK(hipMemcpy(fx.d_rhs0, rhs0 ? rhs0 : z.data(), (size_t)ncol * sizeof(double), hipMemcpyHostToDevice));
    const int64_t nn = h->mm.nfixcol + ncol;
    if ((rc = grow_pair(h, h->mm.d_bfix, h->mm.d_sum_bfix, h->mm.nfixcol, nn))) return rc;
    h->mm.nfixcol = nn;
    if (set_id) *set_id = (int32_t)h->mm.fix.size();
    h->mm.fix.push_back(std::move(fx));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_fixed(ngp_handle *h, double *b, double *sum_b, int64_t *ncols_total) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (ncols_total) *ncols_total = h->mm.nfixcol;
    if (h->mm.nfixcol == 0) return NGP_OK;
    HCHK(hipStreamSynchronize(h->stream));
    if (b) HCHK(hipMemcpy(b, h->mm.d_bfix, (size_t)h->mm.nfixcol * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_b) HCHK(hipMemcpy(sum_b, h->mm.d_sum_bfix, (size_t)h->mm.nfixcol * sizeof(double), hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_fixed(ngp_handle *h, const double *b, const double *sum_b, int64_t ncols_total) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(ncols_total == h->mm.nfixcol, NGP_ERR_ARG, "fixed-effect column count mismatch");
    if (h->mm.nfixcol == 0) return NGP_OK;
    HCHK(hipStreamSynchronize(h->stream));
    if (b) HCHK(hipMemcpy(h->mm.d_bfix, b, (size_t)h->mm.nfixcol * sizeof(double), hipMemcpyHostToDevice));
    if (sum_b) HCHK(hipMemcpy(h->mm.d_sum_bfix, sum_b, (size_t)h->mm.nfixcol * sizeof(double), hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

}  // extern "C"

namespace {
uint64_t bytes_digest(uint64_t x, const void *p, size_t n) {  // FNV-1a, continued from x
    const unsigned char *c = (const unsigned char *)p;
    for (size_t k = 0; k < n; k++) { x ^= c[k]; x *= 1099511628211ull; }
    return x;
}
template <class T>
int upload(ngp_handle *h, DevArray<T> &d, const std::vector<T> &v) {
    int rc;
    if ((rc = d.alloc(h, v.size()))) return rc;
    if (!v.empty()) HCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return NGP_OK;
}
// Host set-up of a sparse fixed-effect set from its CSC arrays (rows strictly ascending inside a column; weights already applied):
//   rptr/rcol/rval   X by records, per record its columns ascending
//   xptr/xcol/xval   X'X by rows, columns ascending: entry (a, c) is fma-accumulated over the records in ascending order from 0.0 --
//                    the bits of the dense set's x0 (a zero product is a no-op there)
//   diagR            the ridged diagonal: X'X[a][a] + min_a |X'X[a][a]| / 10000 (src/mme.jl:149-152)
//   order/dptr       the columns by (Gauss-Seidel depth, column): depth(a) = 1 + max depth(c) over the stored c < a of row a, else 0
struct FixSparseHost {
    std::vector<long long> rptr, xptr, dptr;
    std::vector<int> rcol, xcol, order;
    std::vector<double> rval, xval, diagR;
};
void fixed_sparse_host(int64_t N, int64_t ncol, const std::vector<long long> &cp, const std::vector<int> &cr, const std::vector<double> &cv,
                       FixSparseHost &H) {
    const size_t nnz = cr.size();
    H.rptr.assign((size_t)N + 1, 0);
    for (size_t k = 0; k < nnz; k++) H.rptr[(size_t)cr[k] + 1]++;
    for (int64_t i = 0; i < N; i++) H.rptr[(size_t)i + 1] += H.rptr[(size_t)i];
    H.rcol.resize(nnz); H.rval.resize(nnz);
    {
        std::vector<long long> pos(H.rptr.begin(), H.rptr.end() - 1);
        for (int64_t a = 0; a < ncol; a++)  // columns in ascending order: every record's columns come out ascending
            for (long long k = cp[(size_t)a]; k < cp[(size_t)a + 1]; k++) {
                const long long p = pos[(size_t)cr[(size_t)k]]++;
                H.rcol[(size_t)p] = (int)a; H.rval[(size_t)p] = cv[(size_t)k];
            }
    }
    // the lower triangle row by row: row a's entries (a, c <= a) through a workspace over the columns
    std::vector<double> w((size_t)ncol, 0.0);
    std::vector<char> mark((size_t)ncol, 0);
    std::vector<int> touched;
    std::vector<long long> lptr((size_t)ncol + 1, 0);
    std::vector<int> lcol;
    std::vector<double> lval;
    for (int64_t a = 0; a < ncol; a++) {
        touched.clear();
        for (long long k = cp[(size_t)a]; k < cp[(size_t)a + 1]; k++) {  // the records of column a, ascending
            const int i = cr[(size_t)k];
            const double xa = cv[(size_t)k];
            for (long long p = H.rptr[(size_t)i]; p < H.rptr[(size_t)i + 1]; p++) {
                const int c = H.rcol[(size_t)p];
                if (c > a) break;
                if (!mark[(size_t)c]) { mark[(size_t)c] = 1; touched.push_back(c); }
                w[(size_t)c] = std::fma(xa, H.rval[(size_t)p], w[(size_t)c]);
            }
        }
        std::sort(touched.begin(), touched.end());
        for (int c : touched) {
            lcol.push_back(c); lval.push_back(w[(size_t)c]);
            w[(size_t)c] = 0.0; mark[(size_t)c] = 0;
        }
        lptr[(size_t)a + 1] = (long long)lcol.size();
    }
    // both triangles: row r = its lower entries and diagonal, then the mirrored (a, r) of the rows a > r in ascending a
    H.xptr.assign((size_t)ncol + 1, 0);
    for (int64_t a = 0; a < ncol; a++)
        for (long long k = lptr[(size_t)a]; k < lptr[(size_t)a + 1]; k++) {
            H.xptr[(size_t)a + 1]++;
            if (lcol[(size_t)k] != a) H.xptr[(size_t)lcol[(size_t)k] + 1]++;
        }
    for (int64_t a = 0; a < ncol; a++) H.xptr[(size_t)a + 1] += H.xptr[(size_t)a];
    H.xcol.resize((size_t)H.xptr[(size_t)ncol]); H.xval.resize((size_t)H.xptr[(size_t)ncol]);
    {
        std::vector<long long> pos(H.xptr.begin(), H.xptr.end() - 1);
        for (int64_t a = 0; a < ncol; a++)
            for (long long k = lptr[(size_t)a]; k < lptr[(size_t)a + 1]; k++) {
                const long long p = pos[(size_t)a]++;
                H.xcol[(size_t)p] = lcol[(size_t)k]; H.xval[(size_t)p] = lval[(size_t)k];
            }
        for (int64_t a = 0; a < ncol; a++)
            for (long long k = lptr[(size_t)a]; k < lptr[(size_t)a + 1]; k++) {
                const int c = lcol[(size_t)k];
                if (c == a) continue;
                const long long p = pos[(size_t)c]++;
                H.xcol[(size_t)p] = (int)a; H.xval[(size_t)p] = lval[(size_t)k];
            }
    }
    // ridge and depths (the diagonal is the last entry of a lower row: every column has an entry)
    H.diagR.resize((size_t)ncol);
    for (int64_t a = 0; a < ncol; a++) H.diagR[(size_t)a] = lval[(size_t)lptr[(size_t)a + 1] - 1];
    double mn = std::fabs(H.diagR[0]);
    for (int64_t a = 1; a < ncol; a++) mn = std::min(mn, std::fabs(H.diagR[(size_t)a]));
    for (int64_t a = 0; a < ncol; a++) H.diagR[(size_t)a] += mn / 10000.0;
    std::vector<int> dep((size_t)ncol, 0);
    int maxd = 0;
    for (int64_t a = 0; a < ncol; a++) {
        int d = 0;
        for (long long k = lptr[(size_t)a]; k < lptr[(size_t)a + 1] - 1; k++) d = std::max(d, dep[(size_t)lcol[(size_t)k]] + 1);
        dep[(size_t)a] = d; maxd = std::max(maxd, d);
    }
    H.dptr.assign((size_t)maxd + 2, 0);
    for (int64_t a = 0; a < ncol; a++) H.dptr[(size_t)dep[(size_t)a] + 1]++;
    for (int d = 0; d <= maxd; d++) H.dptr[(size_t)d + 1] += H.dptr[(size_t)d];
    H.order.resize((size_t)ncol);
    std::vector<long long> pos(H.dptr.begin(), H.dptr.end() - 1);
    for (int64_t a = 0; a < ncol; a++) H.order[(size_t)pos[(size_t)dep[(size_t)a]]++] = (int)a;
}
// digest of a dense K without bringing it to the host: k_dense_digest hashes every row on the device (one fixed order), the q row
// words are folded here.  Done once per matrix; sets that share it share the word.
int dense_digest(ngp_handle *h, const DenseK &dk, uint64_t *out) {
    DevArray<unsigned long long> d_rh;
    int rc;
    if ((rc = d_rh.alloc(h, (size_t)dk.q))) return rc;
    hipLaunchKernelGGL(k_dense_digest, dim3((unsigned)((dk.q + 3) / 4)), dim3(256), 0, h->stream, (const double *)dk.K, (long long)dk.ld, (long long)dk.q, d_rh.get());
    std::vector<unsigned long long> rh((size_t)dk.q);
    HCHK(hipMemcpyAsync(rh.data(), d_rh, rh.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    *out = bytes_digest(1469598103934665603ull, rh.data(), rh.size() * sizeof(unsigned long long));
    return NGP_OK;
}

// levels of N records for a random-effect set: records grouped by level (a stable counting sort, ascending within a level) and
// zpz_l = z_l'z_l (src/mme.jl:193-196): the record count; weighted residuals: sum of w over the level's records in that order (:183-188)
void group_levels(const ngp_handle *h, const int32_t *level, int64_t q, std::vector<long long> &lp, std::vector<int> &lr, std::vector<int> &lv,
                  std::vector<double> &zpz) {
    const int64_t N = h->N;
    lp.assign((size_t)q + 1, 0); lr.resize((size_t)N); lv.resize((size_t)N); zpz.assign((size_t)q, 0.0);
    for (int64_t i = 0; i < N; i++) if (level[i] >= 0) lp[(size_t)level[i] + 1]++;  // (-1: a record without a level, tuple sets only)
    for (int64_t l = 0; l < q; l++) lp[(size_t)l + 1] += lp[(size_t)l];
    {
        std::vector<long long> pos(lp.begin(), lp.end() - 1);
        for (int64_t i = 0; i < N; i++) { if (level[i] >= 0) lr[(size_t)pos[(size_t)level[i]]++] = (int)i; lv[(size_t)i] = level[i]; }
    }
    for (int64_t l = 0; l < q; l++) {
        if (h->h_rw.empty()) { zpz[(size_t)l] = (double)(lp[(size_t)l + 1] - lp[(size_t)l]); continue; }
        double a = 0.0;
        for (long long k = lp[(size_t)l]; k < lp[(size_t)l + 1]; k++) a = a + h->h_rw[(size_t)lr[(size_t)k]];
        zpz[(size_t)l] = a;
    }
}
// K of a random-effect set from the caller's CSR (all three NULL: the identity), checked: rows with their columns ascending (the
// summation order of DESIGN.md), symmetric, finite, with a positive diagonal
int parse_k(ngp_handle *h, int64_t q, const int64_t *k_ptr, const int32_t *k_col, const double *k_val, std::vector<long long> &kp,
            std::vector<int> &kc, std::vector<double> &kv, std::vector<double> &kd, bool &offdiag, bool need_diag = true) {
    kp.assign((size_t)q + 1, 0); kc.clear(); kv.clear(); kd.assign((size_t)q, 0.0);
    offdiag = false;
    const bool ident = !k_ptr && !k_col && !k_val;
    if (ident) {
        kc.resize((size_t)q); kv.assign((size_t)q, 1.0);
        for (int64_t l = 0; l <= q; l++) kp[(size_t)l] = l;
        for (int64_t l = 0; l < q; l++) { kc[(size_t)l] = (int)l; kd[(size_t)l] = 1.0; }
    } else {
        REQUIRE(k_ptr[0] == 0, NGP_ERR_ARG, "random-effect set: k_ptr[0] must be 0");
        for (int64_t l = 0; l < q; l++) REQUIRE(k_ptr[l + 1] >= k_ptr[l], NGP_ERR_ARG, "random-effect set: k_ptr must not decrease");
        const int64_t nnz = k_ptr[q];
        REQUIRE(nnz <= ((int64_t)1 << 31), NGP_ERR_ARG, "random-effect set: K has too many entries");
        kc.resize((size_t)nnz); kv.resize((size_t)nnz);
        std::vector<std::pair<int, double>> row;
        for (int64_t l = 0; l < q; l++) {
            row.clear();
            for (int64_t k = k_ptr[l]; k < k_ptr[l + 1]; k++) {
                REQUIRE(k_col[k] >= 0 && (int64_t)k_col[k] < q, NGP_ERR_ARG, "random-effect set: a column of K is outside 0..q-1");
                REQUIRE(std::isfinite(k_val[k]), NGP_ERR_ARG, "random-effect set: non-finite entry in K");
                row.emplace_back(k_col[k], k_val[k]);
            }
            std::sort(row.begin(), row.end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });
            bool diag = false;
            for (size_t k = 0; k < row.size(); k++) {
                REQUIRE(k == 0 || row[k].first != row[k - 1].first, NGP_ERR_ARG, "random-effect set: K has a repeated entry");
                kc[(size_t)k_ptr[l] + k] = row[k].first; kv[(size_t)k_ptr[l] + k] = row[k].second;
                if (row[k].first == l) { diag = true; kd[(size_t)l] = row[k].second; }
                else offdiag = true;
            }
            // (need_diag false: S of a hybrid set, whose trailing diagonal may live in the dense block alone; its caller checks K_ll > 0)
            REQUIRE(!need_diag || (diag && kd[(size_t)l] > 0.0), NGP_ERR_ARG, "random-effect set: every diagonal entry of K must be present and > 0");
            kp[(size_t)l] = k_ptr[l];
        }
        kp[(size_t)q] = nnz;
        for (int64_t l = 0; l < q; l++)  // symmetry: K[l][c] == K[c][l] exactly (row c is sorted: binary search)
            for (long long k = kp[(size_t)l]; k < kp[(size_t)l + 1]; k++) {
                const int c = kc[(size_t)k];
                const auto b = kc.begin() + kp[(size_t)c], e = kc.begin() + kp[(size_t)c + 1];
                const auto it = std::lower_bound(b, e, (int)l);
                REQUIRE(it != e && *it == (int)l && kv[(size_t)(it - kc.begin())] == kv[(size_t)k], NGP_ERR_ARG, "random-effect set: K is not symmetric");
            }
    }
    return NGP_OK;
}

// the launches of one step of the level schedule (ngp_random.h) from the depth of every row: the rows by (depth, row), a depth of more
// than NGP_RS_FUSE_ROWS rows a launch of its own, a run of narrower depths one launch
int plan_schedule(ngp_handle *h, HRand &R, const std::vector<int> &dep) {
    const int64_t q = (int64_t)dep.size();  // (the set's q; the head rows of a hybrid set)
    int rc, maxd = 0;
    for (int64_t l = 0; l < q; l++) maxd = std::max(maxd, dep[(size_t)l]);
    std::vector<int> ord((size_t)q);
    const int nd = maxd + 1;
    std::vector<long long> dp((size_t)nd + 1, 0);
    for (int64_t l = 0; l < q; l++) dp[(size_t)dep[(size_t)l] + 1]++;
    for (int d = 0; d < nd; d++) dp[(size_t)d + 1] += dp[(size_t)d];
    {
        std::vector<long long> pos(dp.begin(), dp.end() - 1);
        for (int64_t l = 0; l < q; l++) ord[(size_t)pos[(size_t)dep[(size_t)l]]++] = (int)l;
    }
    int run0 = -1;
    for (int d = 0; d < nd; d++) {
        if (dp[(size_t)d + 1] - dp[(size_t)d] > NGP_RS_FUSE_ROWS) {
            if (run0 >= 0) R.plan.push_back({0, run0, d, dp[(size_t)run0], dp[(size_t)d]});
            run0 = -1;
            R.plan.push_back({1, d, d + 1, dp[(size_t)d], dp[(size_t)d + 1]});
        } else if (run0 < 0) run0 = d;
    }
    if (run0 >= 0) R.plan.push_back({0, run0, nd, dp[(size_t)run0], dp[(size_t)nd]});
    R.ndepth = nd;
    if ((rc = upload(h, R.d_order, ord)) || (rc = upload(h, R.d_dptr, dp))) return rc;
    return NGP_OK;
}
// k x k (row-major, symmetric) positive definite?  Cholesky on the host, k <= NGP_KMAX
bool host_spd(const double *S, int k) {
    double L[NGP_KMAX * NGP_KMAX] = {0.0};
    for (int i = 0; i < k; i++)
        for (int j = 0; j <= i; j++) {
            double s = S[i * k + j];
            for (int m = 0; m < j; m++) s -= L[i * k + m] * L[j * k + m];
            if (i == j) { if (!(s > 0.0)) return false; L[i * k + i] = std::sqrt(s); }
            else L[i * k + j] = s / L[j * k + j];
        }
    return true;
}

// A random-effect set with a CSR K and k components, behind the argument checks of ngp_add_random_set (k = 1, every level >= 0,
// sdf = scale df) and ngp_add_random_set_tuple (level k x N component-major, -1 allowed).  k = 1 is the (1|g) set of ngp_random.h;
// k > 1 the set of ngp_random_tuple.h: per component the records by level, the k x k blocks W_lc of the header (the diagonal ones
// dense per level, the others CSR with ascending columns; under weighted residuals sums of w in ascending record order), and
// the level schedule over the union of the patterns of K and of the off-diagonal blocks.
int add_random_csr(ngp_handle *h, const int32_t *level, int k, int64_t q, const int64_t *k_ptr, const int32_t *k_col, const double *k_val,
                   double df, const double *scaleM, const double *varU0M, int32_t *set_id) {
    int rc;
    const int64_t N = h->N;
    const int kk = k * k;
    std::vector<long long> kp;
    std::vector<int> kc;
    std::vector<double> kv, kd;
    bool offdiag = false;
    if ((rc = parse_k(h, q, k_ptr, k_col, k_val, kp, kc, kv, kd, offdiag))) return rc;
    HRand R;
    R.q = q; R.tk = k; R.df = df; R.offdiag = offdiag;
    R.scaleM.assign(scaleM, scaleM + kk); R.varU0M.assign(varU0M, varU0M + kk);
    std::vector<long long> lp;
    std::vector<int> lr, lv;
    std::vector<double> zpz;
    std::vector<int> dep((size_t)q, 0);
    if (k == 1) {
        R.sdf = scaleM[0]; R.scale = scaleM[0] / df; R.varU0 = varU0M[0];
        group_levels(h, level, q, lp, lr, lv, zpz);
        if ((rc = upload(h, R.d_zpz, zpz))) return rc;
        for (int64_t l = 0; l < q; l++) {  // the level schedule (ngp_random.h): depths from the sorted rows
            int d = 0;
            for (long long p = kp[(size_t)l]; p < kp[(size_t)l + 1] && kc[(size_t)p] < l; p++) d = std::max(d, dep[(size_t)kc[(size_t)p]] + 1);
            dep[(size_t)l] = d;
        }
    } else {
        R.offdiag = true;  // (a tuple set always runs a Gauss-Seidel engine: its off-diagonal W blocks couple levels even under a diagonal K)
        lp.assign((size_t)k * ((size_t)q + 1), 0); lr.assign((size_t)k * (size_t)N, 0); lv.assign(level, level + (size_t)k * (size_t)N);
        for (int m = 0; m < k; m++) {  // component m's records by level: a stable counting sort, positions into lr from m N
            long long *P = lp.data() + (size_t)m * ((size_t)q + 1);
            const int32_t *lm = level + (size_t)m * (size_t)N;
            for (int64_t i = 0; i < N; i++) if (lm[i] >= 0) P[(size_t)lm[i] + 1]++;
            P[0] = (long long)m * N;
            for (int64_t l = 0; l < q; l++) P[(size_t)l + 1] += P[(size_t)l];
            std::vector<long long> pos(P, P + q);
            for (int64_t i = 0; i < N; i++) if (lm[i] >= 0) lr[(size_t)pos[(size_t)lm[i]]++] = (int)i;
        }
        // the W blocks: per record i (ascending) and pair (a, b) with both levels known, w_i into block (level_a(i), level_b(i)), entry [a][b]
        std::vector<double> wd((size_t)q * (size_t)kk, 0.0);
        std::vector<std::map<int, std::array<double, NGP_KMAX * NGP_KMAX>>> wrow((size_t)q);
        for (int64_t i = 0; i < N; i++) {
            const double w = h->h_rw.empty() ? 1.0 : h->h_rw[(size_t)i];
            for (int a = 0; a < k; a++) {
                const int la = level[(size_t)a * (size_t)N + (size_t)i];
                if (la < 0) continue;
                for (int b = 0; b < k; b++) {
                    const int lb = level[(size_t)b * (size_t)N + (size_t)i];
                    if (lb < 0) continue;
                    if (la == lb) { double &x = wd[(size_t)la * (size_t)kk + (size_t)(a * k + b)]; x = x + w; continue; }
                    auto it = wrow[(size_t)la].find(lb);
                    if (it == wrow[(size_t)la].end()) it = wrow[(size_t)la].emplace(lb, std::array<double, NGP_KMAX * NGP_KMAX>{}).first;
                    double &x = it->second[(size_t)(a * k + b)];
                    x = x + w;
                }
            }
        }
        std::vector<long long> wp((size_t)q + 1, 0);
        std::vector<int> wc;
        std::vector<double> wv;
        for (int64_t l = 0; l < q; l++) {
            for (auto &e : wrow[(size_t)l]) { wc.push_back(e.first); wv.insert(wv.end(), e.second.begin(), e.second.begin() + kk); }
            wp[(size_t)l + 1] = (long long)wc.size();
        }
        REQUIRE(wc.size() < ((size_t)1 << 31) / (size_t)kk, NGP_ERR_ARG, "tuple random-effect set: too many pairs of levels linked by records");
        for (int64_t l = 0; l < q; l++) {  // depths over the union of the two patterns (both rows have ascending columns)
            int d = 0;
            for (long long p = kp[(size_t)l]; p < kp[(size_t)l + 1] && kc[(size_t)p] < l; p++) d = std::max(d, dep[(size_t)kc[(size_t)p]] + 1);
            for (long long p = wp[(size_t)l]; p < wp[(size_t)l + 1] && wc[(size_t)p] < l; p++) d = std::max(d, dep[(size_t)wc[(size_t)p]] + 1);
            dep[(size_t)l] = d;
        }
        if (wc.empty()) { wc.push_back(0); wv.assign((size_t)kk, 0.0); }  // (no empty device arrays)
        if ((rc = upload(h, R.d_wd, wd)) || (rc = upload(h, R.d_wptr, wp)) || (rc = upload(h, R.d_wcol, wc)) || (rc = upload(h, R.d_wval, wv)) ||
            (rc = upload(h, R.d_scaleM, R.scaleM)))
            return rc;
    }
    if (R.offdiag && (rc = plan_schedule(h, R, dep))) return rc;
    R.sig = bytes_digest(bytes_digest(bytes_digest(bytes_digest(1469598103934665603ull, lv.data(), lv.size() * 4), kp.data(), kp.size() * 8), kc.data(),
                                      kc.size() * 4), kv.data(), kv.size() * 8);
    const size_t qk = (size_t)q * (size_t)k, nscr = k == 1 ? (size_t)NGP_RS_ROWS * (size_t)q : tup_scr_len(q, k);
    std::vector<double> vu((size_t)2 * (size_t)kk, 0.0);
    std::copy(R.varU0M.begin(), R.varU0M.end(), vu.begin());
    if ((rc = upload(h, R.d_lptr, lp)) || (rc = upload(h, R.d_lrows, lr)) || (rc = upload(h, R.d_level, lv)) || (rc = upload(h, R.d_kptr, kp)) ||
        (rc = upload(h, R.d_kcol, kc)) || (rc = upload(h, R.d_kval, kv)) || (rc = upload(h, R.d_kdiag, kd)) || (rc = upload(h, R.d_vu, vu)))
        return rc;
    if ((rc = R.d_u.alloc(h, qk)) || (rc = R.d_sum_u.alloc(h, qk)) || (rc = R.d_scr.alloc(h, nscr))) return rc;
    hipError_t e = hipMemset(R.d_u, 0, qk * sizeof(double));
    if (e == hipSuccess) e = hipMemset(R.d_sum_u, 0, qk * sizeof(double));
    if (e == hipSuccess) e = hipMemset(R.d_scr, 0, nscr * sizeof(double));
    if (e == hipSuccess && R.offdiag)
        e = hipFuncSetAttribute(k == 1 ? (const void *)k_rand_gs : (const void *)k_tup_gs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NGP_LDS_MAX);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("add_random_set: ") + hipGetErrorString(e));
    if (set_id) *set_id = (int32_t)h->mm.rnd.size();
    h->mm.rnd.push_back(std::move(R));
    return NGP_OK;
}
}  // namespace

extern "C" {

/* A fixed-effect set given as a sparse matrix: a factor of many levels, or a block of crossed factors and covariates (sampleb!,
 * src/functions.jl:22-36; X'X + min|diag| / 10000, src/mme.jl:149-152).  CSC: col_ptr (ncol + 1), row (strictly ascending inside a
 * column), val.  It takes its place among the fixed-effect sets in the order added and is, bit for bit, the dense set of the same
 * design wherever both exist ("Sparse fixed-effect sets").  Every argument is checked before anything changes. */
int32_t ngp_add_fixed_set_sparse(ngp_handle *h, int64_t N, int64_t ncol, const int64_t *col_ptr, const int32_t *row, const double *val,
                                 int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open: x'x and the Gram window exist after ngp_end_panel");
    REQUIRE(col_ptr && row && val && N == h->N && ncol >= 2 && ncol <= ((int64_t)1 << 20), NGP_ERR_ARG,
            "sparse fixed-effect set: N rows, 2..2^20 columns (a single column is a dense set: ngp_add_fixed_set)");
    REQUIRE(h->mm.fix.size() < 16, NGP_ERR_ARG, "at most 16 fixed-effect sets");
    REQUIRE(col_ptr[0] == 0, NGP_ERR_ARG, "sparse fixed-effect set: col_ptr[0] must be 0");
    for (int64_t a = 0; a < ncol; a++) {
        REQUIRE(col_ptr[a + 1] > col_ptr[a], NGP_ERR_ARG, "sparse fixed-effect set: column " + std::to_string(a) + " has no entry (or col_ptr descends)");
        REQUIRE(col_ptr[a + 1] < ((int64_t)1 << 31), NGP_ERR_ARG, "sparse fixed-effect set: 2^31 entries or more");
    }
    const int64_t nnz = col_ptr[ncol];
    std::vector<long long> cp((size_t)ncol + 1);
    std::vector<int> cr((size_t)nnz);
    std::vector<double> cv((size_t)nnz);
    for (int64_t a = 0; a <= ncol; a++) cp[(size_t)a] = (long long)col_ptr[a];
    for (int64_t a = 0; a < ncol; a++)
        for (int64_t k = col_ptr[a]; k < col_ptr[a + 1]; k++) {
            const int64_t i = row[k];
            REQUIRE(i >= 0 && i < N, NGP_ERR_ARG, "sparse fixed-effect set: row index outside 0 .. N - 1");
            REQUIRE(k == col_ptr[a] || (int64_t)row[k - 1] < i, NGP_ERR_ARG, "sparse fixed-effect set: the rows of column " + std::to_string(a) + " are not strictly ascending");
            REQUIRE(std::isfinite(val[k]), NGP_ERR_ARG, "non-finite value in a fixed-effect column");
            cr[(size_t)k] = (int)i;
            cv[(size_t)k] = h->h_rw.empty() ? val[k] : std::sqrt(h->h_rw[(size_t)i]) * val[k];  // weighted residuals: X~ = s X, the multiply of k_row_scale
        }
    HFix fx;
    fx.sparse = true; fx.ncol = ncol; fx.off = h->mm.nfixcol;
    FixSparseHost H;
    fixed_sparse_host(N, ncol, cp, cr, cv, H);
    int run0 = -1;  // the launches: a depth of more than NGP_FS_FUSE_ROWS columns on its own, a run of narrower depths in one workgroup
    const int nd = (int)H.dptr.size() - 1;
    for (int d = 0; d < nd; d++) {
        if (H.dptr[(size_t)d + 1] - H.dptr[(size_t)d] > NGP_FS_FUSE_ROWS) {
            if (run0 >= 0) fx.plan.push_back({0, run0, d, H.dptr[(size_t)run0], H.dptr[(size_t)d]});
            run0 = -1;
            fx.plan.push_back({1, d, d + 1, H.dptr[(size_t)d], H.dptr[(size_t)d + 1]});
        } else if (run0 < 0) run0 = d;
    }
    if (run0 >= 0) fx.plan.push_back({0, run0, nd, H.dptr[(size_t)run0], H.dptr[(size_t)nd]});
    if ((rc = upload(h, fx.d_cptr, cp)) || (rc = upload(h, fx.d_crow, cr)) || (rc = upload(h, fx.d_cval, cv))) return rc;
    if ((rc = upload(h, fx.d_rptr, H.rptr)) || (rc = upload(h, fx.d_rcol, H.rcol)) || (rc = upload(h, fx.d_rval, H.rval))) return rc;
    if ((rc = upload(h, fx.d_xptr, H.xptr)) || (rc = upload(h, fx.d_xcol, H.xcol)) || (rc = upload(h, fx.d_xval, H.xval))) return rc;
    if ((rc = upload(h, fx.d_diagR, H.diagR)) || (rc = upload(h, fx.d_order, H.order)) || (rc = upload(h, fx.d_dptr, H.dptr))) return rc;
    if ((rc = fx.d_scr.alloc(h, (size_t)NGP_FS_ROWS * (size_t)ncol))) return rc;
    const int64_t nn = h->mm.nfixcol + ncol;
    if ((rc = grow_pair(h, h->mm.d_bfix, h->mm.d_sum_bfix, h->mm.nfixcol, nn))) return rc;
    h->mm.nfixcol = nn;
    if (set_id) *set_id = (int32_t)h->mm.fix.size();
    h->mm.fix.push_back(std::move(fx));
    return NGP_OK;
    NGP_CATCH(h)
}

/* A (1|g) random-effect set (src/mme.jl:165-272; sampled by sampleZ!, src/functions.jl:57-72, 92-97, 498-501).  Every argument is
 * checked before anything changes: a refused call leaves the handle as it was. */
int32_t ngp_add_random_set(ngp_handle *h, const int32_t *level, int64_t q, const int64_t *k_ptr, const int32_t *k_col, const double *k_val,
                           double df, double scale, double varU0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open (ngp_end_panel)");
    REQUIRE(level != nullptr && q >= 1 && q < ((int64_t)1 << 31), NGP_ERR_ARG, "random-effect set: levels of N records and 1 <= q < 2^31");
    REQUIRE(h->mm.rnd.size() < 16, NGP_ERR_ARG, "at most 16 random-effect sets");
    REQUIRE(std::isfinite(df) && df > 0.0 && std::isfinite(scale) && scale >= 0.0, NGP_ERR_ARG, "random-effect set: df > 0 and scale >= 0, finite");
    REQUIRE(std::isfinite(varU0) && varU0 > 0.0, NGP_ERR_ARG, "random-effect set: varU0 must be finite and > 0");
    const bool ident = !k_ptr && !k_col && !k_val;
    REQUIRE(ident || (k_ptr && k_col && k_val), NGP_ERR_ARG, "random-effect set: K as CSR (k_ptr, k_col, k_val), or all three NULL for the identity");
    const int64_t N = h->N;
    for (int64_t i = 0; i < N; i++) REQUIRE(level[i] >= 0 && (int64_t)level[i] < q, NGP_ERR_ARG, "random-effect set: a record's level is outside 0..q-1");
    const double sdf = scale * df;
    return add_random_csr(h, level, 1, q, k_ptr, k_col, k_val, df, &sdf, &varU0, set_id);
    NGP_CATCH(h)
}

/* A correlated (Tuple) random-effect set (src/mme.jl:207-239; sampled by sampleZ!(::Tuple), src/functions.jl:75-89, 100-110, 503-506): k
 * components over one K with a k x k covariance -- (ID, Dam), direct and maternal effects over one pedigree.  level is k x N,
 * component-major, -1 for a record without a level in that component (an unknown dam: the all-zero row of Z).  scale and varU0 are
 * k x k row-major, symmetric positive definite; the caller passes df = 3 + k and scale = v (df - k - 1) (src/mme.jl:265-271).  k = 1 is
 * ngp_add_random_set's chain bit for bit with scale_tuple = scale * df.  The step draws the exact Gibbs conditional, NOT the
 * reference's lines: see the header.  Every argument is checked before anything changes. */
int32_t ngp_add_random_set_tuple(ngp_handle *h, const int32_t *level, int32_t k, int64_t q, const int64_t *k_ptr, const int32_t *k_col,
                                 const double *k_val, double df, const double *scale, const double *varU0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open (ngp_end_panel)");
    REQUIRE(k >= 1 && k <= NGP_KMAX, NGP_ERR_ARG, "tuple random-effect set: 1 <= k <= 4 components");
    REQUIRE(level != nullptr && q >= 1 && q < ((int64_t)1 << 31) / k, NGP_ERR_ARG, "tuple random-effect set: k x N levels and 1 <= q, q k < 2^31");
    REQUIRE(h->mm.rnd.size() < 16, NGP_ERR_ARG, "at most 16 random-effect sets");
    REQUIRE(scale != nullptr && varU0 != nullptr, NGP_ERR_ARG, "tuple random-effect set: scale and varU0 are k x k matrices");
    REQUIRE(std::isfinite(df) && df > 0.0, NGP_ERR_ARG, "tuple random-effect set: df > 0, finite");
    for (int a = 0; a < k * k; a++) REQUIRE(std::isfinite(scale[a]) && std::isfinite(varU0[a]), NGP_ERR_ARG, "tuple random-effect set: non-finite entry in scale or varU0");
    for (int a = 0; a < k; a++)
        for (int b = 0; b < a; b++)
            REQUIRE(scale[a * k + b] == scale[b * k + a] && varU0[a * k + b] == varU0[b * k + a], NGP_ERR_ARG, "tuple random-effect set: scale and varU0 must be symmetric");
    REQUIRE(host_spd(scale, k) && host_spd(varU0, k), NGP_ERR_ARG, "tuple random-effect set: scale and varU0 must be positive definite");
    const bool ident = !k_ptr && !k_col && !k_val;
    REQUIRE(ident || (k_ptr && k_col && k_val), NGP_ERR_ARG, "random-effect set: K as CSR (k_ptr, k_col, k_val), or all three NULL for the identity");
    const int64_t N = h->N;
    for (int64_t i = 0; i < (int64_t)k * N; i++)
        REQUIRE(level[i] >= -1 && (int64_t)level[i] < q, NGP_ERR_ARG, "tuple random-effect set: a record's level is outside 0..q-1 (-1: no level in that component)");
    return add_random_csr(h, level, (int)k, q, k_ptr, k_col, k_val, df, scale, varU0, set_id);
    NGP_CATCH(h)
}

int32_t ngp_get_random(ngp_handle *h, int32_t set_id, double *u, double *sum_u, double *varU, double *sum_varU) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    const HRand &R = h->mm.rnd[(size_t)set_id];
    REQUIRE(R.tk == 1, NGP_ERR_ARG, "a correlated (Tuple) random-effect set: its state is k-fold (ngp_get_random_tuple)");
    HCHK(hipStreamSynchronize(h->stream));
    double vu[2];
    HCHK(hipMemcpy(vu, R.d_vu, sizeof(vu), hipMemcpyDeviceToHost));
    if (u) HCHK(hipMemcpy(u, R.d_u, (size_t)R.q * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_u) HCHK(hipMemcpy(sum_u, R.d_sum_u, (size_t)R.q * sizeof(double), hipMemcpyDeviceToHost));
    if (varU) *varU = vu[0];
    if (sum_varU) *sum_varU = vu[1];
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_random(ngp_handle *h, int32_t set_id, const double *u, const double *sum_u, double varU, double sum_varU) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    REQUIRE(std::isfinite(varU) && varU > 0.0 && std::isfinite(sum_varU), NGP_ERR_ARG, "varU must be finite and > 0, sum_varU finite");
    const HRand &R = h->mm.rnd[(size_t)set_id];
    REQUIRE(R.tk == 1, NGP_ERR_ARG, "a correlated (Tuple) random-effect set: its state is k-fold (ngp_set_random_tuple)");
    if (u) for (int64_t l = 0; l < R.q; l++) REQUIRE(std::isfinite(u[l]), NGP_ERR_ARG, "non-finite random effect");
    if (sum_u) for (int64_t l = 0; l < R.q; l++) REQUIRE(std::isfinite(sum_u[l]), NGP_ERR_ARG, "non-finite sum of a random effect");
    HCHK(hipStreamSynchronize(h->stream));
    const double vu[2] = {varU, sum_varU};
    HCHK(hipMemcpy(R.d_vu, vu, sizeof(vu), hipMemcpyHostToDevice));
    if (u) HCHK(hipMemcpy(R.d_u, u, (size_t)R.q * sizeof(double), hipMemcpyHostToDevice));
    if (sum_u) HCHK(hipMemcpy(R.d_sum_u, sum_u, (size_t)R.q * sizeof(double), hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Fine seam of one random-effect set: sampleZ!(zSet, Z, u, ycorr, varE, varU) of src/functions.jl:92-97 on the caller's arrays (ycorr N,
 * u q, varU one double; updated in place), keyed like ngp_sweep_set (the set's own call counter is the iteration of its draws). */
int32_t ngp_sample_random_set(ngp_handle *h, int32_t set_id, double varE, double *ycorr, double *u, double *varU) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    REQUIRE(ycorr && u && varU, NGP_ERR_ARG, "null state pointer");
    REQUIRE(std::isfinite(varE) && varE > 0.0, NGP_ERR_ARG, "varE must be finite and positive");
    REQUIRE(std::isfinite(*varU) && *varU > 0.0, NGP_ERR_ARG, "varU must be finite and positive");
    HRand &R = h->mm.rnd[(size_t)set_id];
    REQUIRE(R.tk == 1, NGP_ERR_ARG, "a correlated (Tuple) random-effect set: its state is k-fold (ngp_sample_random_set_tuple)");
    for (int64_t l = 0; l < R.q; l++) REQUIRE(std::isfinite(u[l]), NGP_ERR_ARG, "non-finite random effect");
    const uint64_t it = ++R.fine_calls;
    HCHK(hipStreamSynchronize(h->stream));
    double vin[2];
    HCHK(hipMemcpy(vin, R.d_vu, sizeof(vin), hipMemcpyDeviceToHost));
    vin[0] = *varU;  // (the sum of varU stays)
    HCHK(hipMemcpyAsync(h->cm.d_ycorr, ycorr, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, false);  // weighted residuals: the caller's ycorr into y~ = s ycorr
    HCHK(hipMemcpyAsync(R.d_u, u, (size_t)R.q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(R.d_vu, vin, sizeof(vin), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_set_varE, dim3(1), dim3(1), 0, h->stream, h->cm.d_scal, varE);
    launch_random(h, (int)set_id, it);
    if (h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, true);  // ... and back (d_ycorr is scratch here)
    HCHK(hipMemcpyAsync(ycorr, h->cm.d_ycorr, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipMemcpyAsync(u, R.d_u, (size_t)R.q * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipMemcpyAsync(varU, R.d_vu, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    return check_abort(h);
    NGP_CATCH(h)
}

/* State of a random-effect set of k components (ngp_add_random_set_tuple; a set of ngp_add_random_set is k = 1): u and sum_u are q x k with
 * the k components of a level adjacent, varU and sum_varU k x k row-major.  Any pointer may be NULL. */
int32_t ngp_get_random_tuple(ngp_handle *h, int32_t set_id, double *u, double *sum_u, double *varU, double *sum_varU) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    const HRand &R = h->mm.rnd[(size_t)set_id];
    const size_t qk8 = (size_t)R.q * (size_t)R.tk * sizeof(double), kk = (size_t)R.tk * (size_t)R.tk;
    HCHK(hipStreamSynchronize(h->stream));
    if (u) HCHK(hipMemcpy(u, R.d_u, qk8, hipMemcpyDeviceToHost));
    if (sum_u) HCHK(hipMemcpy(sum_u, R.d_sum_u, qk8, hipMemcpyDeviceToHost));
    if (varU) HCHK(hipMemcpy(varU, R.d_vu, kk * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_varU) HCHK(hipMemcpy(sum_varU, R.d_vu + kk, kk * sizeof(double), hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

/* ... and its setter; a NULL pointer leaves that part as it is.  varU must be symmetric positive definite. */
int32_t ngp_set_random_tuple(ngp_handle *h, int32_t set_id, const double *u, const double *sum_u, const double *varU, const double *sum_varU) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    const HRand &R = h->mm.rnd[(size_t)set_id];
    const int k = R.tk;
    const size_t qk = (size_t)R.q * (size_t)k, kk = (size_t)k * (size_t)k;
    if (varU) {
        for (size_t a = 0; a < kk; a++) REQUIRE(std::isfinite(varU[a]), NGP_ERR_ARG, "non-finite entry in varU");
        for (int a = 0; a < k; a++)
            for (int b = 0; b < a; b++) REQUIRE(varU[a * k + b] == varU[b * k + a], NGP_ERR_ARG, "varU must be symmetric");
        REQUIRE(host_spd(varU, k), NGP_ERR_ARG, "varU must be positive definite");
    }
    if (sum_varU) for (size_t a = 0; a < kk; a++) REQUIRE(std::isfinite(sum_varU[a]), NGP_ERR_ARG, "non-finite entry in sum_varU");
    if (u) for (size_t l = 0; l < qk; l++) REQUIRE(std::isfinite(u[l]), NGP_ERR_ARG, "non-finite random effect");
    if (sum_u) for (size_t l = 0; l < qk; l++) REQUIRE(std::isfinite(sum_u[l]), NGP_ERR_ARG, "non-finite sum of a random effect");
    HCHK(hipStreamSynchronize(h->stream));
    if (varU) HCHK(hipMemcpy(R.d_vu, varU, kk * sizeof(double), hipMemcpyHostToDevice));
    if (sum_varU) HCHK(hipMemcpy(R.d_vu + kk, sum_varU, kk * sizeof(double), hipMemcpyHostToDevice));
    if (u) HCHK(hipMemcpy(R.d_u, u, qk * sizeof(double), hipMemcpyHostToDevice));
    if (sum_u) HCHK(hipMemcpy(R.d_sum_u, sum_u, qk * sizeof(double), hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Fine seam of one random-effect set of k components: sampleZ!(zSet::Tuple, ...) of src/functions.jl:100-110 on the caller's arrays (ycorr N,
 * u q x k, varU k x k; updated in place) with the exact conditional of the header, keyed like ngp_sample_random_set. */
int32_t ngp_sample_random_set_tuple(ngp_handle *h, int32_t set_id, double varE, double *ycorr, double *u, double *varU) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    REQUIRE(ycorr && u && varU, NGP_ERR_ARG, "null state pointer");
    REQUIRE(std::isfinite(varE) && varE > 0.0, NGP_ERR_ARG, "varE must be finite and positive");
    HRand &R = h->mm.rnd[(size_t)set_id];
    const int k = R.tk;
    const size_t qk = (size_t)R.q * (size_t)k, kk = (size_t)k * (size_t)k;
    for (size_t a = 0; a < kk; a++) REQUIRE(std::isfinite(varU[a]), NGP_ERR_ARG, "non-finite entry in varU");
    for (int a = 0; a < k; a++)
        for (int b = 0; b < a; b++) REQUIRE(varU[a * k + b] == varU[b * k + a], NGP_ERR_ARG, "varU must be symmetric");
    REQUIRE(host_spd(varU, k), NGP_ERR_ARG, "varU must be positive definite");
    for (size_t l = 0; l < qk; l++) REQUIRE(std::isfinite(u[l]), NGP_ERR_ARG, "non-finite random effect");
    const uint64_t it = ++R.fine_calls;
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpyAsync(h->cm.d_ycorr, ycorr, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, false);  // weighted residuals: the caller's ycorr into y~ = s ycorr
    HCHK(hipMemcpyAsync(R.d_u, u, qk * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HCHK(hipMemcpyAsync(R.d_vu, varU, kk * sizeof(double), hipMemcpyHostToDevice, h->stream));  // (the sum of varU stays)
    hipLaunchKernelGGL(k_set_varE, dim3(1), dim3(1), 0, h->stream, h->cm.d_scal, varE);
    launch_random(h, (int)set_id, it);
    if (h->cm.d_rs) launch_rows(h, h->cm.d_ycorr, h->cm.d_ycorr, true);  // ... and back (d_ycorr is scratch here)
    HCHK(hipMemcpyAsync(ycorr, h->cm.d_ycorr, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipMemcpyAsync(u, R.d_u, qk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipMemcpyAsync(varU, R.d_vu, kk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    return check_abort(h);
    NGP_CATCH(h)
}

/* The Gauss-Seidel engine of a CSR random-effect set whose K has off-diagonal entries: 0 automatic, 1 serial (k_rand_gs), 2 level-scheduled
 * (k_rand_sched_*).  Both engines do the same operations on the same values: the choice changes no bit of any result. */
int32_t ngp_set_random_schedule(ngp_handle *h, int32_t set_id, int32_t mode) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    REQUIRE(mode >= 0 && mode <= 2, NGP_ERR_ARG, "random-effect schedule: 0 automatic, 1 serial, 2 level-scheduled");
    HRand &R = h->mm.rnd[(size_t)set_id];
    REQUIRE(R.hyb ? R.hd > 0 : (!R.dk && R.offdiag), NGP_ERR_ARG,
            "random-effect schedule: only a CSR set whose K has off-diagonal entries, or a hybrid set with head rows, runs a Gauss-Seidel engine "
            "(a diagonal K draws every level on its own, a dense K runs the blocked engine)");
    R.sched_mode = mode;
    return NGP_OK;
    NGP_CATCH(h)
}

/* engine: 0 none (diagonal or dense K), 1 serial, 2 level-scheduled -- the one in force; depths of the level schedule (1 for a diagonal K,
 * 0 for a dense one); Gauss-Seidel launches per step with that engine.  Any pointer may be NULL. */
int32_t ngp_get_random_schedule(ngp_handle *h, int32_t set_id, int32_t *engine, int64_t *depths, int64_t *launches) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int32_t)h->mm.rnd.size(), NGP_ERR_ARG, "unknown random-effect set id");
    const HRand &R = h->mm.rnd[(size_t)set_id];
    const bool gs = R.hyb ? R.hd > 0 : (!R.dk && R.offdiag);  // (a hybrid set: the engine, depths and launches of its head rows)
    if (engine) *engine = !gs ? 0 : R.scheduled() ? 2 : 1;
    if (depths) *depths = gs ? R.ndepth : R.dk ? 0 : 1;
    if (launches) *launches = !gs ? 0 : R.scheduled() ? (int64_t)R.plan.size() : 1;
    return NGP_OK;
    NGP_CATCH(h)
}

/* A^-1 of a pedigree by Henderson's rules with inbreeding (host only, no device, no handle).  n animals, parents in front of their
 * offspring; sire / dam are 1-based positions in the same list, 0 = unknown.  F by Meuwissen and Luo's walk up the ancestors of every
 * animal (A_ii = sum_j L_ij^2 D_jj); then, per animal i with its known parents p (one listed twice counts twice):
 *   d = 1 - sum_p (1 + F_p) / 4,  a = 1 / d,  K_ii += a,  K_ip += -a/2,  K_pi += -a/2,  K_pp' += a/4 for every pair (p, p')
 * in animal order, (i, p) and (p, i) by the same additions: K is reproducible and exactly symmetric.  CSR out, columns ascending. */
int32_t ngp_pedigree_ainv(int64_t n, const int32_t *sire, const int32_t *dam, double *f_out, int64_t *k_ptr, int32_t *k_col, double *k_val,
                          int64_t cap, int64_t *nnz_out) {
    NGP_TRY
    ngp_handle *h = nullptr;  // (messages go where ngp_create's go: ngp_last_error(NULL))
    REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && sire && dam, NGP_ERR_ARG, "pedigree: 1 <= n < 2^31 animals with their sires and dams");
    REQUIRE(cap >= 0 && (cap == 0 || (k_col && k_val)), NGP_ERR_ARG, "pedigree: k_col and k_val hold cap entries");
    for (int64_t i = 0; i < n; i++) {
        REQUIRE(sire[i] >= 0 && (int64_t)sire[i] <= n && dam[i] >= 0 && (int64_t)dam[i] <= n, NGP_ERR_ARG, "pedigree: a parent is outside 0..n");
        REQUIRE((int64_t)sire[i] != i + 1 && (int64_t)dam[i] != i + 1, NGP_ERR_ARG, "pedigree: an animal is its own parent");
        REQUIRE((int64_t)sire[i] <= i && (int64_t)dam[i] <= i, NGP_ERR_ARG, "pedigree: parents must come in front of their offspring");
    }
    auto parents = [&](int64_t i, int64_t p[2]) { int np = 0; if (sire[i]) p[np++] = sire[i] - 1; if (dam[i]) p[np++] = dam[i] - 1; return np; };
    // inbreeding: D_jj = 1 - sum_p (1 + F_p) / 4; ancestors of i from the youngest to the oldest, L_ij carried along
    std::vector<double> F((size_t)n), D((size_t)n), L((size_t)n, 0.0);
    std::priority_queue<int64_t> anc;
    for (int64_t i = 0; i < n; i++) {
        int64_t p[2];
        const int np = parents(i, p);
        double dd = 1.0;
        for (int k = 0; k < np; k++) dd = dd - (1.0 + F[(size_t)p[k]]) / 4.0;
        D[(size_t)i] = dd;
        double aii = 0.0;
        L[(size_t)i] = 1.0;
        anc.push(i);
        while (!anc.empty()) {
            const int64_t j = anc.top();
            anc.pop();
            int64_t pj[2];
            const int nj = parents(j, pj);
            const double lj = L[(size_t)j];
            for (int k = 0; k < nj; k++) {
                if (L[(size_t)pj[k]] == 0.0) anc.push(pj[k]);  // (L of a listed ancestor is > 0: every contribution is)
                L[(size_t)pj[k]] = L[(size_t)pj[k]] + 0.5 * lj;
            }
            aii = aii + lj * lj * D[(size_t)j];
            L[(size_t)j] = 0.0;
        }
        F[(size_t)i] = aii - 1.0;
    }
    // structure: the columns each row is ever given, sorted and made unique
    std::vector<int64_t> cnt((size_t)n + 1, 0);
    auto each_entry = [&](auto &&fn) {  // every addition of Henderson's rules, in animal order: fn(row, column, animal, weight)
        for (int64_t i = 0; i < n; i++) {
            int64_t p[2];
            const int np = parents(i, p);
            fn(i, i, i, 1.0);
            for (int k = 0; k < np; k++) { fn(i, p[k], i, -0.5); fn(p[k], i, i, -0.5); }
            for (int k = 0; k < np; k++) for (int m = 0; m < np; m++) fn(p[k], p[m], i, 0.25);
        }
    };
    each_entry([&](int64_t r, int64_t, int64_t, double) { cnt[(size_t)r + 1]++; });
    for (int64_t i = 0; i < n; i++) cnt[(size_t)i + 1] += cnt[(size_t)i];
    std::vector<int32_t> cols((size_t)cnt[(size_t)n]);
    {
        std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
        each_entry([&](int64_t r, int64_t c, int64_t, double) { cols[(size_t)pos[(size_t)r]++] = (int32_t)c; });
    }
    std::vector<int64_t> kp((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        const auto b = cols.begin() + cnt[(size_t)i], e = cols.begin() + cnt[(size_t)i + 1];
        std::sort(b, e);
        kp[(size_t)i + 1] = kp[(size_t)i] + (std::unique(b, e) - b);
    }
    const int64_t nnz = kp[(size_t)n];
    if (nnz_out) *nnz_out = nnz;
    if (f_out) std::copy(F.begin(), F.end(), f_out);
    if (k_ptr) std::copy(kp.begin(), kp.end(), k_ptr);
    REQUIRE(cap >= nnz, NGP_ERR_ARG, "pedigree: cap is smaller than the number of entries of A^-1 (nnz_out holds it: call again)");
    for (int64_t i = 0; i < n; i++) std::copy(cols.begin() + cnt[(size_t)i], cols.begin() + cnt[(size_t)i] + (kp[(size_t)i + 1] - kp[(size_t)i]), k_col + kp[(size_t)i]);
    std::fill(k_val, k_val + nnz, 0.0);
    each_entry([&](int64_t r, int64_t c, int64_t i, double w) {
        const int32_t *b = k_col + kp[(size_t)r], *e = k_col + kp[(size_t)r + 1];
        const double a = 1.0 / D[(size_t)i];
        k_val[std::lower_bound(b, e, (int32_t)c) - k_col] += a * w;
    });
    return NGP_OK;
    NGP_CATCH(nullptr)
}

/* A22 = A[idx, idx] of a pedigree without the dense A (host only): Colleau's indirect method, A = T diag(d) T' with T the gene flow
 * (T = I + T P, P the parent matrix with 1/2 entries).  Per listed animal g = idx[j], with x = e_g:
 *   backward, i = g .. 0:  x[sire_i] = x[sire_i] + x[i] / 2;  x[dam_i] = x[dam_i] + x[i] / 2          (x = T' e_g)
 *   x[i] = x[i] * d_i,  d_i = 1, 0.75 - F_p / 4, 0.5 - (F_s + F_d) / 4 with no, one, two known parents
 *   forward, i = 0 .. n - 1:  w[i] = x[i] + (w[sire_i] + w[dam_i]) / 2  (an unknown parent adds 0.0)   (w = T x = A e_g)
 * and A22[j][k] = w[idx[k]] for k >= j, mirrored into A22[k][j]: exactly symmetric.  The columns are spread over min(16, m) threads,
 * column j to thread j mod that count; no column depends on another, so the count changes no bit.  f: the inbreeding coefficients
 * ngp_pedigree_ainv returns.  idx: 0-based positions, any order, repeats allowed. */
int32_t ngp_pedigree_a22(int64_t n, const int32_t *sire, const int32_t *dam, const double *f, const int64_t *idx, int64_t m, double *A22, int64_t ld) {
    NGP_TRY
    ngp_handle *h = nullptr;
    REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && sire && dam && f, NGP_ERR_ARG, "pedigree: 1 <= n < 2^31 animals with their sires, dams and inbreeding coefficients");
    REQUIRE(m >= 1 && idx && A22 && ld >= m, NGP_ERR_ARG, "pedigree A22: m >= 1 listed animals, an m x m output with ld >= m");
    for (int64_t i = 0; i < n; i++) {
        REQUIRE(sire[i] >= 0 && (int64_t)sire[i] <= i && dam[i] >= 0 && (int64_t)dam[i] <= i, NGP_ERR_ARG, "pedigree: parents must come in front of their offspring (0 = unknown)");
        REQUIRE(std::isfinite(f[i]), NGP_ERR_ARG, "pedigree: non-finite inbreeding coefficient");
    }
    for (int64_t j = 0; j < m; j++) REQUIRE(idx[j] >= 0 && idx[j] < n, NGP_ERR_ARG, "pedigree A22: a listed animal is outside 0..n-1");
    std::vector<double> d((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int s = sire[i], dm = dam[i];
        if (s && dm) d[(size_t)i] = 0.5 - (f[(size_t)s - 1] + f[(size_t)dm - 1]) / 4.0;
        else if (s || dm) d[(size_t)i] = 0.75 - f[(size_t)(s ? s : dm) - 1] / 4.0;
        else d[(size_t)i] = 1.0;
    }
    const int nt = (int)std::min<int64_t>(16, m);
    std::vector<std::vector<double>> xs((size_t)nt, std::vector<double>((size_t)n)), ws(xs);  // (allocated here: a thread must not throw)
    auto work = [&](int t) {
        std::vector<double> &x = xs[(size_t)t], &w = ws[(size_t)t];
        for (int64_t j = t; j < m; j += nt) {
            const int64_t g = idx[j];
            std::fill(x.begin(), x.end(), 0.0);
            x[(size_t)g] = 1.0;
            for (int64_t i = g; i >= 0; i--) {
                const double hx = x[(size_t)i] / 2.0;
                if (hx == 0.0) continue;
                if (sire[i]) x[(size_t)sire[i] - 1] = x[(size_t)sire[i] - 1] + hx;
                if (dam[i]) x[(size_t)dam[i] - 1] = x[(size_t)dam[i] - 1] + hx;
            }
            for (int64_t i = 0; i <= g; i++) x[(size_t)i] = x[(size_t)i] * d[(size_t)i];
            for (int64_t i = 0; i < n; i++) {
                const double ws = sire[i] ? w[(size_t)sire[i] - 1] : 0.0, wd = dam[i] ? w[(size_t)dam[i] - 1] : 0.0;
                w[(size_t)i] = x[(size_t)i] + (ws + wd) / 2.0;
            }
            for (int64_t k = j; k < m; k++) A22[(size_t)j * (size_t)ld + (size_t)k] = w[(size_t)idx[k]];
        }
    };
    {
        struct Joiner {  // (a std::thread constructor that throws must not unwind past joinable threads)
            std::vector<std::thread> th;
            ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); }
        } pool;
        for (int t = 1; t < nt; t++) pool.th.emplace_back(work, t);
        work(0);
    }
    for (int64_t j = 0; j < m; j++)
        for (int64_t k = j + 1; k < m; k++) A22[(size_t)k * (size_t)ld + (size_t)j] = A22[(size_t)j * (size_t)ld + (size_t)k];
    return NGP_OK;
    NGP_CATCH(nullptr)
}

/* Kept samples to a binary file WITHOUT stopping the chain (the reference appends text rows at every kept iteration,
 * src/samplers.jl:56-104, src/outFiles.jl:17-21: 10 MB of text per sample at P = 600,000).  From the next ngp_run on, every kept
 * iteration (ngp_set_schedule) leaves one record: packed on the device into a ring of four slots, copied to pinned host memory on a
 * second stream and written by a thread of the library's own; ngp_run returns when its last record is in the file.  path == NULL
 * closes the file.  The file: ngp_state.h.  nextgp.jl_amd/api.py (samples_to_out_files) turns it into the reference's *Out text files. */
/* BayesLV marker set (include/nextgp_hip.h).  On the device the set is a BayesPR set with one variance per locus and NO region entry
 * (h_regs / segments): k_prep draws no region chi-square for it and k_regdraw never touches it; its variances come from launch_lv. */
int32_t ngp_add_marker_set_lv(ngp_handle *h, int64_t col0, int64_t ncol, double varBeta0, const double *C, int64_t ld, int32_t ncov,
                              double varZeta0, int32_t est_mode, double est_fraction, const double *zeta0, const double *lhs0,
                              const double *rhs0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = check_marker_slot(h, col0, ncol, ncol, "marker set outside the panel"))) return rc;
    REQUIRE(ncov >= 1 && ncov <= NGP_LV_MAXCOV, NGP_ERR_ARG, "BayesLV: the covariate matrix needs 1..16 columns");
    REQUIRE(C != nullptr && ld >= ncol, NGP_ERR_ARG, "BayesLV: covariates missing (ncol x ncov, column-major, ld >= ncol)");
    REQUIRE(std::isfinite(varBeta0) && varBeta0 > 0.0, NGP_ERR_ARG, "BayesLV: varBeta0 must be finite and positive (its logarithm is modelled)");
    REQUIRE(std::isfinite(varZeta0) && varZeta0 > 0.0, NGP_ERR_ARG, "BayesLV: varZeta0 must be finite and positive");
    REQUIRE(est_mode >= 0 && est_mode <= 2, NGP_ERR_ARG, "BayesLV: est_mode is 0 (fixed), 1 (var(zeta)) or 2 (fraction of var(logVar))");
    if (est_mode == 2) REQUIRE(std::isfinite(est_fraction) && est_fraction > 0.0, NGP_ERR_ARG, "BayesLV: est_fraction must be positive in mode 2");
    if (est_mode != 0) REQUIRE(ncol >= 2, NGP_ERR_ARG, "BayesLV: an estimated varZeta needs at least two loci (a sample variance)");
    for (int k = 0; k < ncov; k++)
        for (int64_t l = 0; l < ncol; l++) REQUIRE(std::isfinite(C[(size_t)k * ld + l]), NGP_ERR_ARG, "BayesLV: non-finite covariate");
    if (zeta0) for (int64_t l = 0; l < ncol; l++) REQUIRE(std::isfinite(zeta0[l]), NGP_ERR_ARG, "BayesLV: non-finite zeta0");
    std::vector<double> inv;
    if ((rc = lv_icpc(h, C, ld, ncol, ncov, inv))) return rc;
    HLv V;
    V.set = (int)h->sets.size(); V.n = ncol; V.ncov = ncov; V.mode = est_mode; V.frac = (est_mode == 2) ? est_fraction : 0.0; V.varZeta0 = varZeta0;
    if (zeta0) V.zeta0.assign(zeta0, zeta0 + ncol);
    const size_t nseg = (size_t)((ncol + 255) / 256);
    if ((rc = V.d_C.alloc(h, (size_t)ncol * ncov))) return rc;
    if ((rc = V.d_iCpC.alloc(h, inv.size()))) return rc;
    if ((rc = V.d_zeta.alloc(h, (size_t)ncol))) return rc;
    if ((rc = V.d_logv.alloc(h, (size_t)ncol))) return rc;
    if ((rc = V.d_part.alloc(h, nseg * (size_t)ncov))) return rc;
    if ((rc = V.d_vpart.alloc(h, nseg))) return rc;
    if ((rc = V.d_st.alloc(h, NGP_LV_WORDS))) return rc;
    if ((rc = V.d_trapseg.alloc(h, nseg))) return rc;
    for (int k = 0; k < ncov; k++)
        HCHK(hipMemcpy(V.d_C + (size_t)k * ncol, C + (size_t)k * ld, (size_t)ncol * sizeof(double), hipMemcpyHostToDevice));
    HCHK(hipMemcpy(V.d_iCpC, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = lv_reset(h, V))) return rc;
    // the marker set: BayesPR with one variance per locus, outside the region tables (df, scale: never read -- no region draw)
    MarkerSetSpec sp;
    sp.hs = HSet{col0, ncol, NGP_METHOD_BAYESLV, 4.0, 0.0, ncol, h->nvb, 0, 0, 0.5, std::vector<double>((size_t)ncol, varBeta0)};
    sp.hs.lv = (int)h->mm.lv.size();
    sp.ds = dset(NGP_METHOD_BAYESPR, 0, 4.0, 0.0, col0, ncol);
    column_loci(sp, h->nvb, 1);
    sp.lhs0 = lhs0; sp.rhs0 = rhs0;
    sp.lv = &V;
    return commit_marker_set(h, sp, set_id);
    NGP_CATCH(h)
}

int32_t ngp_get_lv_state(ngp_handle *h, int32_t set_id, double *c, double *sum_c, double *varZeta, double *sum_varZeta, double *zeta,
                         double *iCpC, int64_t *trapped) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int)h->sets.size() && h->sets[(size_t)set_id].lv >= 0, NGP_ERR_ARG, "not a BayesLV set");
    const HLv &V = h->mm.lv[(size_t)h->sets[(size_t)set_id].lv];
    HCHK(hipStreamSynchronize(h->stream));
    double st[NGP_LV_WORDS];
    HCHK(hipMemcpy(st, V.d_st, sizeof(st), hipMemcpyDeviceToHost));
    for (int k = 0; k < V.ncov; k++) {
        if (c) c[k] = st[NGP_LV_C + k];
        if (sum_c) sum_c[k] = st[NGP_LV_SUM + k];
    }
    if (varZeta) *varZeta = st[NGP_LV_VZ];
    if (sum_varZeta) *sum_varZeta = st[NGP_LV_SUM + NGP_LV_VZ];
    if (trapped) *trapped = (int64_t)st[NGP_LV_TRAP];
    if (zeta) HCHK(hipMemcpy(zeta, V.d_zeta, (size_t)V.n * sizeof(double), hipMemcpyDeviceToHost));
    if (iCpC) HCHK(hipMemcpy(iCpC, V.d_iCpC, (size_t)V.ncov * V.ncov * sizeof(double), hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_lv_state(ngp_handle *h, int32_t set_id, const double *c, const double *sum_c, double varZeta, double sum_varZeta,
                         const double *zeta) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(set_id >= 0 && set_id < (int)h->sets.size() && h->sets[(size_t)set_id].lv >= 0, NGP_ERR_ARG, "not a BayesLV set");
    REQUIRE(std::isfinite(varZeta) && varZeta > 0.0 && std::isfinite(sum_varZeta), NGP_ERR_ARG, "BayesLV: varZeta must be finite and positive");
    HLv &V = h->mm.lv[(size_t)h->sets[(size_t)set_id].lv];
    if (zeta) for (int64_t l = 0; l < V.n; l++) REQUIRE(std::isfinite(zeta[l]), NGP_ERR_ARG, "BayesLV: non-finite zeta");
    HCHK(hipStreamSynchronize(h->stream));
    double st[NGP_LV_WORDS];
    HCHK(hipMemcpy(st, V.d_st, sizeof(st), hipMemcpyDeviceToHost));
    for (int k = 0; k < V.ncov; k++) {
        if (c) st[NGP_LV_C + k] = c[k];
        if (sum_c) st[NGP_LV_SUM + k] = sum_c[k];
    }
    st[NGP_LV_VZ] = varZeta; st[NGP_LV_SUM + NGP_LV_VZ] = sum_varZeta;
    HCHK(hipMemcpy(V.d_st, st, sizeof(st), hipMemcpyHostToDevice));
    if (zeta) HCHK(hipMemcpy(V.d_zeta, zeta, (size_t)V.n * sizeof(double), hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_sample_file(ngp_handle *h, const char *path) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    HCHK(hipStreamSynchronize(h->stream));
    h->smp.reset();
    if (!path) return NGP_OK;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    auto S = std::make_unique<SampleStream>();
    S->path = path; S->device = h->device;
    S->f.reset(std::fopen(path, "wb"));
    if (!S->f) return fail(h, NGP_ERR_ARG, std::string("cannot open the sample file for writing: ") + path);
    hipError_t e = hipStreamCreate(&S->copy_stream);
    for (int i = 0; i < SampleStream::NSLOT && e == hipSuccess; i++) {
        e = hipEventCreateWithFlags(&S->ev_packed[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&S->ev_copied[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("sample stream: ") + hipGetErrorString(e));
    S->writer = std::thread(sample_writer_loop, S.get());
    h->smp = std::move(S);
    return NGP_OK;
    NGP_CATCH(h)
}

/* Placement census of the last persistent-sweep launch of this handle: out[b] = (XCC id + 1) << 32 | HW_REG_HW_ID of workgroup b,
 * 0 for a workgroup that never became resident (n >= grid entries; *grid = 1 sampler + reducers + streamers); *retries = launches of
 * this handle that ended at the census (grid not co-resident beside another chain's) and were run again with the device to
 * themselves; *exclusive = whether the handle's calls now lease the whole device. */
int32_t ngp_get_census(ngp_handle *h, uint64_t *out, int64_t n, int64_t *grid, int64_t *retries, int32_t *exclusive) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && h->plan.mode == 1, NGP_ERR_STATE, "no persistent sweep on this handle");
    const int64_t g = h->last_grid > 0 ? h->last_grid : sweep_grid(h->plan);
    if (grid) *grid = g;
    if (retries) *retries = h->census_retries;
    if (exclusive) *exclusive = h->exclusive ? 1 : 0;
    if (out) {
        REQUIRE(n >= g, NGP_ERR_ARG, "census buffer smaller than the grid");
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipMemcpy(out, h->cm.d_census_tbl, (size_t)g * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return NGP_OK;
    NGP_CATCH(h)
}

/* The warmer of the last persistent-sweep launch (role_warmer, ngp_sweep.h): *active = 1 if workgroup NG shared the sampler's XCD and
 * warmed its L2 in place of the streamers, *blocks = blocks it warmed.  Both are zero where there was no candidate. */
int32_t ngp_get_warmer(ngp_handle *h, int32_t *active, int64_t *blocks) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && h->plan.mode == 1, NGP_ERR_STATE, "no persistent sweep on this handle");
    unsigned w[3] = {0, 0, 0};
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(w, h->cm.d_ccnt + h->cm.census_off + 8, sizeof(w), hipMemcpyDeviceToHost));
    if (active) *active = w[1] ? 1 : 0;
    if (blocks) *blocks = (int64_t)w[2];
    return NGP_OK;
    NGP_CATCH(h)
}

/* Test hook of the census fallback: the sweep of iteration `iteration` (1-based, as ngp_get_state counts) closes its own census as
 * "timed out" -- what a grid that is not co-resident does after 20 ms -- so that the retry path (abort before any role has run,
 * kernels behind it skipped, whole-device lease, the iteration resumed from k_prep) can be exercised on one chain.  0 = off. */
int32_t ngp_debug_fail_census(ngp_handle *h, int64_t iteration) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(iteration >= 0, NGP_ERR_ARG, "iteration must be >= 0");
    h->dbg_census_fail_iter = iteration;
    if (iteration > 0) h->exclusive = false;
    return NGP_OK;
    NGP_CATCH(h)
}

/* Test hook of ngp_allreduce_posterior's grouping: the handle is treated as living on device `vdev` (-1: its real device) when
 * leaders are chosen and buffers packed / unpacked -- with several handles of ONE GPU given different virtual devices the
 * multi-device branch runs up to the collective itself, which is then a sum on that one device instead of ncclAllReduce. */
int32_t ngp_debug_set_virtual_device(ngp_handle *h, int32_t vdev) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(vdev >= -1 && vdev < 64, NGP_ERR_ARG, "virtual device: -1 (off) or 0..63");
    h->vdev = vdev;
    return NGP_OK;
    NGP_CATCH(h)
}

/* Test hook of the staged loaders (tests/test_gpu_ingest.py): every host loop that stages a caller's matrix or a panel file through a
 * fixed-size buffer (256 MiB of columns, 64 MiB of blocks) takes `bytes` for that size instead, so that a panel of a few hundred
 * columns crosses many chunk boundaries.  Each loop rounds as before (one column, one 64-column block, 64 GRM columns at least).
 * 0 = the defaults. */
int32_t ngp_debug_set_staging_bytes(ngp_handle *h, int64_t bytes) {
    NGP_TRY
    int rc;
    if ((rc = enter(h, true))) return rc;
    REQUIRE(bytes >= 0, NGP_ERR_ARG, "staging bytes: 0 (the defaults) or a positive size");
    h->dbg_staging_bytes = bytes;
    return NGP_OK;
    NGP_CATCH(h)
}

/* Test hook of the exception barrier (tests/test_abi.py): throws inside an entry point, past the same NGP_TRY / NGP_CATCH every
 * other one runs in.  kind 0: std::bad_alloc, 1: std::length_error (a std::vector asked for more than max_size), 2: a
 * non-standard exception.  h may be NULL (the message then goes where ngp_create's go).  Never returns NGP_OK. */
int32_t ngp_debug_throw(ngp_handle *h, int32_t kind) {
    NGP_TRY
    if (kind == 0) throw std::bad_alloc();
    if (kind == 1) { std::vector<double> v; v.resize(v.max_size() + 1); }
    if (kind == 2) throw 42;
    return fail(h, NGP_ERR_ARG, "ngp_debug_throw: kind must be 0, 1 or 2");
    NGP_CATCH(h)
}

}  // extern "C"

/* ---- GBLUP (src/prepMatVec.jl:122-126): the genomic relationship matrix on the device, its inverse, dense random-effect sets, and
 * handles without a genotype panel.  Kernels and summation orders: ngp_dense.h, DESIGN.md section 2. ---- */
namespace {
// rocSOLVER (Cholesky factorisation and inverse of G) is loaded on first use, like RCCL: no link-time dependency
struct RocSolver {
    void *lib = nullptr;
    int (*CreateHandle)(void **) = nullptr;
    int (*DestroyHandle)(void *) = nullptr;
    int (*SetStream)(void *, hipStream_t) = nullptr;
    int (*Dpotrf)(void *, int, int, double *, int, int *) = nullptr;
    int (*Dpotri)(void *, int, int, double *, int, int *) = nullptr;
    std::string err;
    std::mutex mu;
    bool load() {
        std::lock_guard<std::mutex> lk(mu);
        if (lib) return true;
        const char *names[] = {"librocsolver.so.0", "librocsolver.so", "/opt/rocm/lib/librocsolver.so.0", "/opt/rocm/lib/librocsolver.so"};
        for (const char *nm : names) { lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
        if (!lib) { const char *d = dlerror(); err = std::string("cannot load rocSOLVER: ") + (d ? d : "?"); return false; }
        CreateHandle = (decltype(CreateHandle))dlsym(lib, "rocblas_create_handle");
        DestroyHandle = (decltype(DestroyHandle))dlsym(lib, "rocblas_destroy_handle");
        SetStream = (decltype(SetStream))dlsym(lib, "rocblas_set_stream");
        Dpotrf = (decltype(Dpotrf))dlsym(lib, "rocsolver_dpotrf");
        Dpotri = (decltype(Dpotri))dlsym(lib, "rocsolver_dpotri");
        if (!CreateHandle || !DestroyHandle || !SetStream || !Dpotrf || !Dpotri) { err = "rocSOLVER symbols missing"; dlclose(lib); lib = nullptr; return false; }
        return true;
    }
} g_rocsolver;
constexpr int ROCBLAS_FILL_LOWER = 122;

// a range of raw genotype columns into G: staged in chunks of whole columns (256 MiB, multiples of 64 columns), centred (and scaled)
// in fp64 on the device, then G += Xc Xc' on the matrix cores
template <typename TIn>
int grm_columns(ngp_handle *h, const TIn *M, int64_t ncol, int64_t ld) {
    int rc;
    if ((rc = enter(h))) return rc;
    Grm &g = h->grm;
    REQUIRE(g.state == 1, NGP_ERR_STATE, "ngp_grm_columns_* needs an open relationship matrix (ngp_grm_begin)");
    REQUIRE(M != nullptr && ncol > 0, NGP_ERR_ARG, "genotype columns: a matrix of at least one column");
    REQUIRE(ld >= g.N, NGP_ERR_ARG, "leading dimension smaller than N");
    const int64_t N = g.N, Npad = g.m->ld;
    int64_t cchunk = std::min<int64_t>((ncol + 63) / 64 * 64, staging_bytes(h, (int64_t)256 << 20) / (int64_t)(std::max<int64_t>(ld, Npad) * (int64_t)sizeof(double)));
    cchunk = std::max<int64_t>(64, cchunk / 64 * 64);
    DevArray<TIn> d_g;
    DevArray<double> d_xc, d_tp;
    DevArray<unsigned> d_bad;
    if (d_g.alloc_raw((size_t)cchunk * (size_t)ld) != hipSuccess || d_xc.alloc_raw((size_t)cchunk * (size_t)Npad) != hipSuccess)
        return fail(h, NGP_ERR_NOMEM, "staging buffers of the relationship matrix");
    if ((rc = d_tp.alloc(h, (size_t)cchunk)) || (rc = d_bad.alloc(h, 2))) return rc;
    std::vector<double> tp((size_t)cchunk);
    double sum2pq = g.sum2pq;
    const int64_t col_base = g.ncols;  // columns of the calls before this one (g.ncols moves on with every chunk)
    const unsigned nb64 = (unsigned)(Npad / 64);
    for (int64_t c0 = 0; c0 < ncol; c0 += cchunk) {
        const int64_t nc = std::min<int64_t>(cchunk, ncol - c0), cpad = (nc + 3) / 4 * 4;
        const unsigned bad0[2] = {0u, 0xFFFFFFFFu};
        hipError_t e = hipMemcpyAsync(d_bad, bad0, sizeof(bad0), hipMemcpyHostToDevice, h->stream);
        // (the last column may be shorter than ld in the caller's buffer: nc - 1 full columns + N elements)
        if (e == hipSuccess) e = hipMemcpyAsync(d_g, M + (size_t)c0 * (size_t)ld, ((size_t)(nc - 1) * (size_t)ld + (size_t)N) * sizeof(TIn), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_grm_cols<TIn>, dim3((unsigned)cpad), dim3(64), 0, h->stream, (const TIn *)d_g, (long long)N, (long long)ld, (long long)nc,
                               (long long)Npad, g.method, d_xc.get(), d_tp.get(), d_bad.get());
            unsigned bad[2] = {0u, 0u};
            e = hipMemcpyAsync(bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(tp.data(), d_tp, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            // a refused chunk has not touched G: the columns of the calls (and chunks) before it stay, the builder stays open
            if (e == hipSuccess && bad[0] != 0u) return fail(h, NGP_ERR_ARG, "non-finite genotype value in the columns of the relationship matrix");
            if (e == hipSuccess && bad[1] != 0xFFFFFFFFu)
                return fail(h, NGP_ERR_ARG, "relationship matrix, method 2: column " + std::to_string(col_base + c0 + (int64_t)bad[1] - 1) +
                                                " (0-based, counted over all calls) is monomorphic: 2 p (1 - p) = 0 divides 0 by 0 (src/misc.jl:152-154)");
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_grm_syrk, dim3(nb64, nb64), dim3(256), 0, h->stream, (const double *)d_xc, (long long)Npad, (long long)cpad, g.m->K.get());
            e = hipStreamSynchronize(h->stream);  // the staging buffers are reused by the next chunk
        }
        if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("relationship matrix columns: ") + hipGetErrorString(e));
        if (g.method == 1) for (int64_t c = 0; c < nc; c++) sum2pq = sum2pq + tp[(size_t)c];
        g.sum2pq = sum2pq;
        g.ncols += nc;
    }
    return NGP_OK;
}

}  // namespace

extern "C" {

int32_t ngp_set_records(ngp_handle *h, int64_t N) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->req.storage == NGP_STORAGE_F32, NGP_ERR_ARG, "ngp_set_records: compact storage concerns genotype panels; this handle has none");
    // one inert block of 64 zero columns stands in for the panel: every array a chain has exists, no sweep is ever launched
    const PlanRequest saved = h->req;
    h->req.mode = 0;
    rc = alloc_panel(h, N, NGP_BLK);
    h->req = saved;
    if (rc) return rc;
    h->records_only = true;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_grm_begin(ngp_handle *h, int64_t N, int32_t method) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(N >= 1 && N < ((int64_t)1 << 31) - 64, NGP_ERR_ARG, "relationship matrix: 1 <= N < 2^31");
    REQUIRE(method == 1 || method == 2, NGP_ERR_ARG, "relationship matrix: method 1 or 2 (src/misc.jl:149-156)");
    h->grm = Grm();  // (a matrix begun earlier and never used goes first)
    auto m = std::make_shared<DenseK>();
    const int64_t Npad = (N + 63) / 64 * 64;
    if ((rc = m->K.alloc(h, (size_t)Npad * (size_t)Npad))) return rc;
    HCHK(hipStreamSynchronize(h->stream));
    m->q = N; m->ld = Npad;
    h->grm.m = std::move(m); h->grm.state = 1; h->grm.method = method; h->grm.N = N;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_grm_columns_f64(ngp_handle *h, const double *M, int64_t ncol, int64_t ld) {
    NGP_TRY
    return grm_columns<double>(h, M, ncol, ld);
    NGP_CATCH(h)
}

int32_t ngp_grm_columns_f32(ngp_handle *h, const float *M, int64_t ncol, int64_t ld) {
    NGP_TRY
    return grm_columns<float>(h, M, ncol, ld);
    NGP_CATCH(h)
}

int32_t ngp_grm_columns_u8(ngp_handle *h, const uint8_t *M, int64_t ncol, int64_t ld) {
    NGP_TRY
    return grm_columns<uint8_t>(h, M, ncol, ld);
    NGP_CATCH(h)
}

int32_t ngp_grm_end(ngp_handle *h) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    Grm &g = h->grm;
    REQUIRE(g.state == 1, NGP_ERR_STATE, "ngp_grm_end needs an open relationship matrix (ngp_grm_begin)");
    REQUIRE(g.ncols > 0, NGP_ERR_STATE, "relationship matrix: no genotype column was given");
    const double denom = g.method == 1 ? g.sum2pq : (double)g.ncols;
    if (!(denom > 0.0) || !std::isfinite(denom)) {
        h->grm = Grm();
        return fail(h, NGP_ERR_ARG, "relationship matrix, method 1: the sum of 2 p (1 - p) over the columns is not positive (every column monomorphic?): "
                                    "G would be 0 / 0 (src/misc.jl:150); the matrix is dropped");
    }
    const unsigned gy = (unsigned)std::min<int64_t>(g.N, 65535);
    hipLaunchKernelGGL(k_grm_mirror, dim3((unsigned)((g.N + 255) / 256), gy), dim3(256), 0, h->stream, g.m->K.get(), (long long)g.N, (long long)g.m->ld, 1, denom);
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    g.state = 2;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_grm_get(ngp_handle *h, double *G_out) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const Grm &g = h->grm;
    REQUIRE(g.state >= 2, NGP_ERR_STATE, "no complete relationship matrix on this handle (ngp_grm_end; a dense set may have taken it)");
    REQUIRE(G_out != nullptr, NGP_ERR_ARG, "null output pointer");
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy2D(G_out, (size_t)g.N * sizeof(double), g.m->K, (size_t)g.m->ld * sizeof(double), (size_t)g.N * sizeof(double), (size_t)g.N, hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_grm_invert(ngp_handle *h) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    Grm &g = h->grm;
    REQUIRE(g.state == 2, NGP_ERR_STATE, g.state == 3 ? "the relationship matrix is inverted already" : "ngp_grm_invert needs a complete relationship matrix (ngp_grm_end)");
    if (!g_rocsolver.load()) return fail(h, NGP_ERR_HIP, g_rocsolver.err + " (ngp_grm_invert factorises on the device; there is no host fallback)");
    struct Blas {  // a rocBLAS handle for this call, destroyed however it ends
        void *p = nullptr;
        ~Blas() { if (p) (void)g_rocsolver.DestroyHandle(p); }
    } blas;
    if (g_rocsolver.CreateHandle(&blas.p) != 0 || !blas.p || g_rocsolver.SetStream(blas.p, h->stream) != 0)
        return fail(h, NGP_ERR_HIP, "rocblas_create_handle / rocblas_set_stream failed");
    DevArray<int> d_info;
    if ((rc = d_info.alloc(h, 1))) return rc;
    int info = 0;
    const int n = (int)g.N, lda = (int)g.m->ld;
    // column-major, lower triangle: what k_grm_syrk computed and k_grm_mirror copied (G is symmetric, either triangle would do)
    int st = g_rocsolver.Dpotrf(blas.p, ROCBLAS_FILL_LOWER, n, g.m->K.get(), lda, d_info.get());
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(&info, d_info, sizeof(int), hipMemcpyDeviceToHost));
    if (st != 0 || info != 0) {  // the factorisation has overwritten part of G: the matrix is gone either way
        h->grm = Grm();
        if (st != 0) return fail(h, NGP_ERR_HIP, "rocsolver_dpotrf failed (rocblas status " + std::to_string(st) + "); the relationship matrix is dropped");
        return fail(h, NGP_ERR_ARG, "the relationship matrix is not positive definite: the Cholesky factorisation failed at pivot " + std::to_string(info) +
                                        " (1-based); the matrix is dropped");
    }
    st = g_rocsolver.Dpotri(blas.p, ROCBLAS_FILL_LOWER, n, g.m->K.get(), lda, d_info.get());
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(&info, d_info, sizeof(int), hipMemcpyDeviceToHost));
    if (st != 0 || info != 0) {
        h->grm = Grm();
        if (st != 0) return fail(h, NGP_ERR_HIP, "rocsolver_dpotri failed (rocblas status " + std::to_string(st) + "); the relationship matrix is dropped");
        return fail(h, NGP_ERR_ARG, "inverse of the relationship matrix: zero pivot " + std::to_string(info) + " (1-based); the matrix is dropped");
    }
    const unsigned gy = (unsigned)std::min<int64_t>(g.N, 65535);
    hipLaunchKernelGGL(k_grm_mirror, dim3((unsigned)((g.N + 255) / 256), gy), dim3(256), 0, h->stream, g.m->K.get(), (long long)g.N, (long long)g.m->ld, 0, 1.0);
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    g.state = 3;
    return NGP_OK;
    NGP_CATCH(h)
}

/* A random-effect set with a dense K (ngp_dense.h).  Every argument is checked before anything changes: a refused call leaves the
 * handle (and its relationship matrix) as it was. */
int32_t ngp_add_random_set_dense(ngp_handle *h, const int32_t *level, int64_t q, const double *K, ngp_handle *k_src, int32_t k_src_set, double df,
                                 double scale, double varU0, int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open (ngp_end_panel)");
    REQUIRE(q >= 1 && q < ((int64_t)1 << 31), NGP_ERR_ARG, "random-effect set: 1 <= q < 2^31");
    REQUIRE(level != nullptr || q == h->N, NGP_ERR_ARG, "random-effect set: level == NULL means record i is level i and needs q == N");
    REQUIRE(h->mm.rnd.size() < 16, NGP_ERR_ARG, "at most 16 random-effect sets");
    REQUIRE(std::isfinite(df) && df > 0.0 && std::isfinite(scale) && scale >= 0.0, NGP_ERR_ARG, "random-effect set: df > 0 and scale >= 0, finite");
    REQUIRE(std::isfinite(varU0) && varU0 > 0.0, NGP_ERR_ARG, "random-effect set: varU0 must be finite and > 0");
    REQUIRE(!(K && k_src), NGP_ERR_ARG, "dense random-effect set: K from a host pointer OR from a set of another handle, not both");
    const int64_t N = h->N;
    std::vector<int32_t> ident;
    if (!level) { ident.resize((size_t)N); for (int64_t i = 0; i < N; i++) ident[(size_t)i] = (int32_t)i; level = ident.data(); }
    for (int64_t i = 0; i < N; i++) REQUIRE(level[i] >= 0 && (int64_t)level[i] < q, NGP_ERR_ARG, "random-effect set: a record's level is outside 0..q-1");
    // where K comes from: a host matrix (copied), a set of another handle (by reference), or this handle's inverted relationship matrix
    std::shared_ptr<DenseK> dk;
    bool from_grm = false;
    if (K) {
        for (int64_t l = 0; l < q; l++)
            for (int64_t c = 0; c <= l; c++) {
                const double a = K[(size_t)l * (size_t)q + (size_t)c];
                REQUIRE(std::isfinite(a), NGP_ERR_ARG, "random-effect set: non-finite entry in K");
                REQUIRE(a == K[(size_t)c * (size_t)q + (size_t)l], NGP_ERR_ARG, "random-effect set: K is not symmetric");
            }
        dk = std::make_shared<DenseK>();
        if (dk->K.alloc_raw((size_t)q * (size_t)q) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "dense K");
        dk->q = q; dk->ld = q;
        HCHK(hipMemcpy(dk->K, K, (size_t)q * (size_t)q * sizeof(double), hipMemcpyHostToDevice));
    } else if (k_src) {
        // (like ngp_share_panel's owner: a complete handle of this device that no other thread is setting up during this call)
        REQUIRE(k_src != h, NGP_ERR_ARG, "dense random-effect set: k_src is this handle (a set shares the K of a set on ANOTHER handle)");
        REQUIRE(k_src->stream != nullptr && k_src->pm && !k_src->panel_open, NGP_ERR_ARG, "dense random-effect set: k_src has no panel or records yet (or its panel is still open)");
        REQUIRE(k_src->device == h->device, NGP_ERR_ARG, "dense random-effect set: a shared K must be on this handle's device");
        REQUIRE(k_src_set >= 0 && k_src_set < (int32_t)k_src->mm.rnd.size() && k_src->mm.rnd[(size_t)k_src_set].dk && !k_src->mm.rnd[(size_t)k_src_set].hyb,
                NGP_ERR_ARG, "dense random-effect set: k_src_set is not a dense set of k_src");
        dk = k_src->mm.rnd[(size_t)k_src_set].dk;
        REQUIRE(dk->q == q, NGP_ERR_ARG, "dense random-effect set: the shared K has another q");
        HCHK(hipStreamSynchronize(k_src->stream));
    } else {
        REQUIRE(h->grm.state == 3, NGP_ERR_STATE, "dense random-effect set without K: this handle has no inverted relationship matrix (ngp_grm_invert)");
        REQUIRE(h->grm.N == q, NGP_ERR_ARG, "dense random-effect set: the relationship matrix has another size than q");
        dk = h->grm.m;
        from_grm = true;
    }
    // the diagonal (k_rand_levels' lhs, k_dense_var) back from the device, and the digest of the whole matrix if nobody has taken it yet
    std::vector<double> kd((size_t)q);
    HCHK(hipMemcpy2D(kd.data(), sizeof(double), dk->K, (size_t)(dk->ld + 1) * sizeof(double), sizeof(double), (size_t)q, hipMemcpyDeviceToHost));
    uint64_t kdig = dk->digest;
    if (!k_src && (rc = dense_digest(h, *dk, &kdig))) return rc;  // (a fresh matrix; the word is stored below, once the call can no longer be refused)
    for (int64_t l = 0; l < q; l++) REQUIRE(std::isfinite(kd[(size_t)l]) && kd[(size_t)l] > 0.0, NGP_ERR_ARG, "random-effect set: every diagonal entry of K must be > 0");
    std::vector<long long> lp;
    std::vector<int> lr, lv;
    std::vector<double> zpz;
    group_levels(h, level, q, lp, lr, lv, zpz);
    HRand R;
    R.q = q; R.df = df; R.scale = scale; R.varU0 = varU0; R.offdiag = true;
    R.sdf = scale * df; R.scaleM = {R.sdf}; R.varU0M = {varU0};
    // digest of the level coding and of every entry of K (hashed on the device: a dense K may never have been on the host)
    R.sig = bytes_digest(bytes_digest(1469598103934665603ull ^ 0x44454E5345ull, lv.data(), lv.size() * 4), &kdig, sizeof(kdig));
    const double vu[2] = {varU0, 0.0};
    if ((rc = upload(h, R.d_lptr, lp)) || (rc = upload(h, R.d_lrows, lr)) || (rc = upload(h, R.d_level, lv)) || (rc = upload(h, R.d_kdiag, kd)) ||
        (rc = upload(h, R.d_zpz, zpz)))
        return rc;
    if ((rc = R.d_u.alloc(h, (size_t)q)) || (rc = R.d_sum_u.alloc(h, (size_t)q)) || (rc = R.d_vu.alloc(h, 2)) ||
        (rc = R.d_scr.alloc(h, (size_t)NGP_RS_ROWS_DENSE * (size_t)q)))
        return rc;
    HCHK(hipMemcpy(R.d_vu, vu, sizeof(vu), hipMemcpyHostToDevice));
    HCHK(hipStreamSynchronize(h->stream));
    dk->digest = kdig;
    R.dk = std::move(dk);
    if (from_grm) h->grm = Grm();  // consumed: the set owns the matrix now
    if (set_id) *set_id = (int32_t)h->mm.rnd.size();
    h->mm.rnd.push_back(std::move(R));
    return NGP_OK;
    NGP_CATCH(h)
}

/* ---- single-step GBLUP: the corner block D = G_w^-1 - A22^-1 on the device, and the hybrid random-effect set (ngp_hybrid.h) ---- */

/* After ngp_grm_end, in place of ngp_grm_invert: G_w = (1 - w) G + w A22 (k_ss_blend), both G_w and A22 inverted by rocSOLVER (A22 in a
 * second N x N buffer, released on return), D = G_w^-1 - A22^-1 on the computed triangle, mirrored.  A refusal by NGP_ERR_ARG (w outside
 * [0, 1), A22 not finite or not symmetric, either matrix not positive definite) drops the matrix; the handle stays usable. */
int32_t ngp_grm_single_step(ngp_handle *h, const double *A22, int64_t ld, double w) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    Grm &g = h->grm;
    REQUIRE(g.state == 2, NGP_ERR_STATE, "ngp_grm_single_step needs a complete relationship matrix that is not inverted yet (ngp_grm_end)");
    REQUIRE(A22 != nullptr && ld >= g.N, NGP_ERR_ARG, "single-step: A22 is N x N with ld >= N");
    const int64_t N = g.N, Npad = g.m->ld;
    bool ok = std::isfinite(w) && w >= 0.0 && w < 1.0;
    const char *why = "single-step: the blending weight w must be in [0, 1); the matrix is dropped";
    for (int64_t i = 0; ok && i < N; i++)
        for (int64_t j = 0; j <= i; j++) {
            const double a = A22[(size_t)i * (size_t)ld + (size_t)j];
            if (!std::isfinite(a) || a != A22[(size_t)j * (size_t)ld + (size_t)i]) { ok = false; why = "single-step: A22 must be finite and exactly symmetric; the matrix is dropped"; break; }
        }
    if (!ok) { h->grm = Grm(); return fail(h, NGP_ERR_ARG, why); }
    if (!g_rocsolver.load()) return fail(h, NGP_ERR_HIP, g_rocsolver.err + " (ngp_grm_single_step factorises on the device; there is no host fallback)");
    struct Blas {  // a rocBLAS handle for this call, destroyed however it ends
        void *p = nullptr;
        ~Blas() { if (p) (void)g_rocsolver.DestroyHandle(p); }
    } blas;
    if (g_rocsolver.CreateHandle(&blas.p) != 0 || !blas.p || g_rocsolver.SetStream(blas.p, h->stream) != 0)
        return fail(h, NGP_ERR_HIP, "rocblas_create_handle / rocblas_set_stream failed");
    DevArray<double> d_a;  // A22, laid out as G is (leading dimension Npad, zero beyond N); released when this call returns
    DevArray<int> d_info;
    if ((rc = d_a.alloc(h, (size_t)Npad * (size_t)Npad)) || (rc = d_info.alloc(h, 1))) return rc;
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy2D(d_a, (size_t)Npad * sizeof(double), A22, (size_t)ld * sizeof(double), (size_t)N * sizeof(double), (size_t)N, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)std::min<int64_t>(N, 65535));
    hipLaunchKernelGGL(k_ss_blend, grid, dim3(256), 0, h->stream, g.m->K.get(), (const double *)d_a, (long long)N, (long long)Npad, 1.0 - w, w);
    // the two inverses, lower triangle, column-major (as ngp_grm_invert): G_w first, then A22
    double *mats[2] = {g.m->K.get(), d_a.get()};
    const char *names[2] = {"G_w = (1 - w) G + w A22", "A22"};
    for (int k = 0; k < 2; k++) {
        int info = 0;
        int st = g_rocsolver.Dpotrf(blas.p, ROCBLAS_FILL_LOWER, (int)N, mats[k], (int)Npad, d_info.get());
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipMemcpy(&info, d_info, sizeof(int), hipMemcpyDeviceToHost));
        if (st == 0 && info == 0) {
            st = g_rocsolver.Dpotri(blas.p, ROCBLAS_FILL_LOWER, (int)N, mats[k], (int)Npad, d_info.get());
            HCHK(hipStreamSynchronize(h->stream));
            HCHK(hipMemcpy(&info, d_info, sizeof(int), hipMemcpyDeviceToHost));
        }
        if (st != 0 || info != 0) {  // the factorisation has overwritten part of the matrix: it is gone either way
            h->grm = Grm();
            if (st != 0) return fail(h, NGP_ERR_HIP, "rocsolver_dpotrf / dpotri failed (rocblas status " + std::to_string(st) + "); the relationship matrix is dropped");
            return fail(h, NGP_ERR_ARG, std::string("single-step: ") + names[k] + " is not positive definite (pivot " + std::to_string(info) +
                                            ", 1-based); the matrix is dropped");
        }
    }
    hipLaunchKernelGGL(k_ss_diff, grid, dim3(256), 0, h->stream, g.m->K.get(), (const double *)d_a, (long long)N, (long long)Npad);
    hipLaunchKernelGGL(k_grm_mirror, grid, dim3(256), 0, h->stream, g.m->K.get(), (long long)N, (long long)Npad, 0, 1.0);
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    g.state = 4;
    return NGP_OK;
    NGP_CATCH(h)
}

/* A random-effect set with K = S + embed(D): S a q x q CSR, D a dense nd x nd block over the LAST nd levels (ngp_hybrid.h).  Every argument
 * is checked before anything changes: a refused call leaves the handle (and its relationship matrix) as it was. */
int32_t ngp_add_random_set_hybrid(ngp_handle *h, const int32_t *level, int64_t q, const int64_t *k_ptr, const int32_t *k_col, const double *k_val,
                                  int64_t nd, const double *D, ngp_handle *k_src, int32_t k_src_set, double df, double scale, double varU0,
                                  int32_t *set_id) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    REQUIRE(!h->panel_open, NGP_ERR_STATE, "the panel is still open (ngp_end_panel)");
    REQUIRE(level != nullptr && q >= 1 && q < ((int64_t)1 << 31), NGP_ERR_ARG, "random-effect set: levels of N records and 1 <= q < 2^31");
    REQUIRE(nd >= 1 && nd <= q, NGP_ERR_ARG, "hybrid random-effect set: the dense block covers the last nd levels, 1 <= nd <= q");
    REQUIRE(h->mm.rnd.size() < 16, NGP_ERR_ARG, "at most 16 random-effect sets");
    REQUIRE(std::isfinite(df) && df > 0.0 && std::isfinite(scale) && scale >= 0.0, NGP_ERR_ARG, "random-effect set: df > 0 and scale >= 0, finite");
    REQUIRE(std::isfinite(varU0) && varU0 > 0.0, NGP_ERR_ARG, "random-effect set: varU0 must be finite and > 0");
    REQUIRE(k_ptr != nullptr && (k_ptr[q] == 0 || (k_col && k_val)), NGP_ERR_ARG, "hybrid random-effect set: S as CSR (k_ptr, k_col, k_val); an empty S needs k_ptr alone");
    REQUIRE(!(D && k_src), NGP_ERR_ARG, "hybrid random-effect set: D from a host pointer OR from a set of another handle, not both");
    const int64_t N = h->N, hd = q - nd;
    for (int64_t i = 0; i < N; i++) REQUIRE(level[i] >= 0 && (int64_t)level[i] < q, NGP_ERR_ARG, "random-effect set: a record's level is outside 0..q-1");
    std::vector<long long> kp;
    std::vector<int> kc;
    std::vector<double> kv, kd;
    bool offdiag = false;
    if ((rc = parse_k(h, q, k_ptr, k_col, k_val, kp, kc, kv, kd, offdiag, false))) return rc;
    // S split: the CSR the engine walks (everything but the trailing x trailing entries) and the entries that go into the dense block
    std::vector<long long> fp((size_t)q + 1, 0);
    std::vector<int> fcol, tr, tc;
    std::vector<double> fval, tv;
    for (int64_t l = 0; l < q; l++) {
        for (long long k = kp[(size_t)l]; k < kp[(size_t)l + 1]; k++) {
            if (l >= hd && kc[(size_t)k] >= hd) { tr.push_back((int)(l - hd)); tc.push_back(kc[(size_t)k] - (int)hd); tv.push_back(kv[(size_t)k]); }
            else { fcol.push_back(kc[(size_t)k]); fval.push_back(kv[(size_t)k]); }
        }
        fp[(size_t)l + 1] = (long long)fcol.size();
    }
    for (int64_t l = 0; l < hd; l++) REQUIRE(kd[(size_t)l] > 0.0, NGP_ERR_ARG, "hybrid random-effect set: every diagonal entry of K must be > 0 (a head row of S lacks one)");
    // where D comes from: a host matrix (copied, S_tt added on the host), a hybrid set of another handle (its T, by reference), or this
    // handle's own corner block (ngp_grm_single_step; S_tt added on the device once nothing can refuse the call any more)
    std::shared_ptr<DenseK> dk;
    bool from_grm = false;
    std::vector<double> td((size_t)nd);  // the diagonal of T
    if (D) {
        std::vector<double> T((size_t)nd * (size_t)nd);
        for (int64_t l = 0; l < nd; l++)
            for (int64_t c = 0; c <= l; c++) {
                const double a = D[(size_t)l * (size_t)nd + (size_t)c];
                REQUIRE(std::isfinite(a), NGP_ERR_ARG, "hybrid random-effect set: non-finite entry in D");
                REQUIRE(a == D[(size_t)c * (size_t)nd + (size_t)l], NGP_ERR_ARG, "hybrid random-effect set: D is not symmetric");
                T[(size_t)l * (size_t)nd + (size_t)c] = a; T[(size_t)c * (size_t)nd + (size_t)l] = a;
            }
        for (size_t e = 0; e < tv.size(); e++) { double &x = T[(size_t)tr[e] * (size_t)nd + (size_t)tc[e]]; x = x + tv[e]; }
        for (int64_t l = 0; l < nd; l++) td[(size_t)l] = T[(size_t)l * (size_t)nd + (size_t)l];
        for (int64_t l = 0; l < nd; l++) REQUIRE(std::isfinite(td[(size_t)l]) && td[(size_t)l] > 0.0, NGP_ERR_ARG, "hybrid random-effect set: every diagonal entry of K must be > 0");
        dk = std::make_shared<DenseK>();
        if (dk->K.alloc_raw((size_t)nd * (size_t)nd) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "dense block of a hybrid set");
        dk->q = nd; dk->ld = nd;
        HCHK(hipMemcpy(dk->K, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice));
    } else if (k_src) {
        REQUIRE(k_src != h, NGP_ERR_ARG, "hybrid random-effect set: k_src is this handle (a set shares the block of a set on ANOTHER handle)");
        REQUIRE(k_src->stream != nullptr && k_src->pm && !k_src->panel_open, NGP_ERR_ARG, "hybrid random-effect set: k_src has no panel or records yet (or its panel is still open)");
        REQUIRE(k_src->device == h->device, NGP_ERR_ARG, "hybrid random-effect set: a shared block must be on this handle's device");
        REQUIRE(k_src_set >= 0 && k_src_set < (int32_t)k_src->mm.rnd.size() && k_src->mm.rnd[(size_t)k_src_set].hyb, NGP_ERR_ARG,
                "hybrid random-effect set: k_src_set is not a hybrid set of k_src");
        dk = k_src->mm.rnd[(size_t)k_src_set].dk;  // (T of that set: its S_tt is in it already; this set's S_tt is taken to be the same)
        REQUIRE(dk->q == nd, NGP_ERR_ARG, "hybrid random-effect set: the shared block has another nd");
        HCHK(hipStreamSynchronize(k_src->stream));
        HCHK(hipMemcpy2D(td.data(), sizeof(double), dk->K, (size_t)(dk->ld + 1) * sizeof(double), sizeof(double), (size_t)nd, hipMemcpyDeviceToHost));
    } else {
        REQUIRE(h->grm.state == 4, NGP_ERR_STATE, "hybrid random-effect set without D: this handle has no single-step corner block (ngp_grm_single_step)");
        REQUIRE(h->grm.N == nd, NGP_ERR_ARG, "hybrid random-effect set: the corner block has another size than nd");
        dk = h->grm.m;
        from_grm = true;
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipMemcpy2D(td.data(), sizeof(double), dk->K, (size_t)(dk->ld + 1) * sizeof(double), sizeof(double), (size_t)nd, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < tv.size(); e++) if (tr[e] == tc[e]) td[(size_t)tr[e]] = td[(size_t)tr[e]] + tv[e];  // (the sum k_hyb_fold forms)
    }
    for (int64_t l = 0; l < nd; l++) REQUIRE(std::isfinite(td[(size_t)l]) && td[(size_t)l] > 0.0, NGP_ERR_ARG, "hybrid random-effect set: every diagonal entry of K must be > 0");
    for (int64_t l = 0; l < nd; l++) kd[(size_t)(hd + l)] = td[(size_t)l];
    std::vector<long long> lp;
    std::vector<int> lr, lv;
    std::vector<double> zpz;
    group_levels(h, level, q, lp, lr, lv, zpz);
    HRand R;
    R.q = q; R.df = df; R.scale = scale; R.varU0 = varU0; R.offdiag = true; R.hyb = true; R.hd = hd;
    R.sdf = scale * df; R.scaleM = {R.sdf}; R.varU0M = {varU0};
    if (hd > 0) {  // the level schedule of the head rows, exactly as ngp_add_random_set plans it: every column c < l of a head row is a head column
        std::vector<int> dep((size_t)hd, 0);
        for (int64_t l = 0; l < hd; l++) {
            int d = 0;
            for (long long p = fp[(size_t)l]; p < fp[(size_t)l + 1] && fcol[(size_t)p] < l; p++) d = std::max(d, dep[(size_t)fcol[(size_t)p]] + 1);
            dep[(size_t)l] = d;
        }
        if ((rc = plan_schedule(h, R, dep))) return rc;
    }
    if (fcol.empty()) { fcol.push_back(0); fval.push_back(0.0); }  // (no empty device arrays; fp says that nothing is stored)
    const double vu[2] = {varU0, 0.0};
    if ((rc = upload(h, R.d_lptr, lp)) || (rc = upload(h, R.d_lrows, lr)) || (rc = upload(h, R.d_level, lv)) || (rc = upload(h, R.d_kptr, fp)) ||
        (rc = upload(h, R.d_kcol, fcol)) || (rc = upload(h, R.d_kval, fval)) || (rc = upload(h, R.d_kdiag, kd)) || (rc = upload(h, R.d_zpz, zpz)))
        return rc;
    if ((rc = R.d_u.alloc(h, (size_t)q)) || (rc = R.d_sum_u.alloc(h, (size_t)q)) || (rc = R.d_vu.alloc(h, 2)) ||
        (rc = R.d_scr.alloc(h, (size_t)NGP_RS_ROWS_HYBRID * (size_t)q)))
        return rc;
    HCHK(hipMemcpy(R.d_vu, vu, sizeof(vu), hipMemcpyHostToDevice));
    if (from_grm && !tv.empty()) {  // T = D + S_tt on the device, one sum per stored entry (nothing below refuses the call on an argument)
        DevArray<int> d_tr, d_tc;
        DevArray<double> d_tv;
        if ((rc = upload(h, d_tr, tr)) || (rc = upload(h, d_tc, tc)) || (rc = upload(h, d_tv, tv))) return rc;
        hipLaunchKernelGGL(k_hyb_fold, dim3((unsigned)((tv.size() + 255) / 256)), dim3(256), 0, h->stream, dk->K.get(), (long long)dk->ld, (long long)tv.size(),
                           (const int *)d_tr, (const int *)d_tc, (const double *)d_tv);
        HCHK(hipStreamSynchronize(h->stream));
    }
    uint64_t kdig = dk->digest;
    if (!k_src && (rc = dense_digest(h, *dk, &kdig))) return rc;
    // the model signature: the level coding and S as a CSR set digests them, then the dense block as a dense set digests it
    R.sig = bytes_digest(bytes_digest(bytes_digest(bytes_digest(1469598103934665603ull ^ 0x485942ull, lv.data(), lv.size() * 4), kp.data(), kp.size() * 8), kc.data(),
                                      kc.size() * 4), kv.data(), kv.size() * 8);
    R.sig = bytes_digest(bytes_digest(R.sig, &nd, sizeof(nd)), &kdig, sizeof(kdig));
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipGetLastError());
    dk->digest = kdig;
    R.dk = std::move(dk);
    if (from_grm) h->grm = Grm();  // consumed: the set owns the block now
    if (set_id) *set_id = (int32_t)h->mm.rnd.size();
    h->mm.rnd.push_back(std::move(R));
    return NGP_OK;
    NGP_CATCH(h)
}

}  // extern "C"

/* ---- prediction panel and prediction results (ngp_predict.h; DESIGN.md section 2, "Prediction") ---- */
namespace {
std::atomic<uint64_t> g_pred_id{0};

// the open prediction panel is abandoned: the handle is as it was without one
void drop_prediction(ngp_handle *h) {
    if (h->pm) h->pm->pred.reset();
    h->pred_open = false;
    h->cm.pred_for = 0; h->cm.pred_rows = 0;
}

int begin_prediction(ngp_handle *h, int64_t Np) {
    REQUIRE(h->pm && !h->panel_open, NGP_ERR_STATE, "a prediction panel needs a finished training panel (ngp_set_panel_* / ngp_end_panel)");
    REQUIRE(!h->records_only, NGP_ERR_STATE, "a records-only (GBLUP) handle has no marker panel to predict from");
    REQUIRE(Np >= 1 && Np <= ((int64_t)1 << 30), NGP_ERR_ARG, "prediction panel: Np must be at least 1");
    auto pp = std::make_shared<PredPanel>();
    pp->Np = Np;
    pp->R = std::min<int64_t>(NGP_PRED_MAXR, (Np + 15) / 16 * 16);
    pp->S = (Np + pp->R - 1) / pp->R;
    pp->id = ++g_pred_id;
    const size_t elems = (size_t)h->NBLK * (size_t)pp->S * (size_t)pp->R * NGP_BLK;
    int rc;
    h->pm->pred.reset();  // (the old one goes first: two never coexist on the device)
    if ((rc = pp->tiles.alloc(h, h->req.storage == 1 ? elems / 4 : elems))) return rc;  // born zero: columns never uploaded stay zero
    if ((rc = pp->mean.alloc(h, (size_t)h->Ppad))) return rc;
    HCHK(hipStreamSynchronize(h->stream));
    h->pm->pred = std::move(pp);
    h->pred_open = true;
    return NGP_OK;
}

template <typename TIn>
int prediction_columns(ngp_handle *h, int64_t col0, const TIn *M, int64_t ncol, int64_t ld, int centre) {
    int rc;
    if ((rc = enter(h, true))) return rc;
    REQUIRE(h->pred_open && h->pm && h->pm->pred, NGP_ERR_STATE, "ngp_prediction_columns_* needs an open prediction panel (ngp_begin_prediction_panel)");
    PredPanel &pp = *h->pm->pred;
    REQUIRE(M != nullptr, NGP_ERR_ARG, "null panel pointer");
    REQUIRE(ld >= pp.Np, NGP_ERR_ARG, "leading dimension smaller than Np");
    REQUIRE(col0 >= 0 && ncol > 0 && col0 + ncol <= h->P, NGP_ERR_ARG, "column range outside the panel");
    REQUIRE(h->req.storage == 0 || sizeof(TIn) == 1, NGP_ERR_ARG, "compact storage takes genotype codes: ngp_prediction_columns_u8 or ngp_load_prediction_file");
    const int64_t Np = pp.Np, Lp = pp.R * pp.S;
    const int64_t cchunk = std::max<int64_t>(1, std::min<int64_t>(ncol, staging_bytes(h, (int64_t)256 << 20) / (int64_t)(ld * sizeof(TIn))));
    DevArray<TIn> d_g;
    DevArray<unsigned> d_bad;
    DevArray<double> d_scr;
    if (d_g.alloc_raw((size_t)cchunk * ld) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "staging buffer");
    if ((rc = d_bad.alloc(h, 1)) || (rc = d_scr.alloc(h, (size_t)cchunk))) return rc;
    hipError_t e = hipSuccess;
    for (int64_t c0 = 0; c0 < ncol && e == hipSuccess; c0 += cchunk) {
        const int64_t nc = std::min<int64_t>(cchunk, ncol - c0);
        e = hipMemcpyAsync(d_g, M + (size_t)c0 * ld, ((size_t)(nc - 1) * ld + (size_t)Np) * sizeof(TIn), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) break;
        // what is subtracted: the TRAINING panel's column means (never means of these rows), or nothing
        double *d_mu = pp.mean + col0 + c0;
        if (centre) e = hipMemcpyAsync(d_mu, h->pm->mean + col0 + c0, (size_t)nc * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
        else e = hipMemsetAsync(d_mu, 0, (size_t)nc * sizeof(double), h->stream);
        if (e != hipSuccess) break;
        if constexpr (sizeof(TIn) != 1)  // (the column sums only flag non-finite values here)
            hipLaunchKernelGGL(k_cols_mean<TIn>, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, h->stream, (const TIn *)d_g, (long long)Np, (long long)ld,
                               (long long)nc, 0, d_scr.get(), d_bad.get());
        if constexpr (sizeof(TIn) == 1) {
            if (h->req.storage == 1)
                hipLaunchKernelGGL(k_cols_fill8, dim3((unsigned)((Lp / 16 + 255) / 256), (unsigned)nc), dim3(256), 0, h->stream, (uint8_t *)pp.tiles.get(),
                                   (const uint8_t *)d_g, (long long)Np, (long long)ld, (long long)(col0 + c0), (int)pp.R, (int)pp.S);
        }
        if (h->req.storage == 0)  // x = (float)((double)v - mu), as the training tiles are formed; residual weights never scale these rows
            hipLaunchKernelGGL(k_cols_fill<TIn>, dim3((unsigned)((Lp / 4 + 255) / 256), (unsigned)nc), dim3(256), 0, h->stream, pp.tiles.get(), (const TIn *)d_g,
                               (long long)Np, (long long)ld, (long long)(col0 + c0), (int)pp.R, (int)pp.S, (const double *)d_mu, (const double *)nullptr);
        e = hipStreamSynchronize(h->stream);  // the staging buffer is reused by the next chunk
    }
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("prediction columns: ") + hipGetErrorString(e));
    REQUIRE(bad == 0u, NGP_ERR_ARG, "non-finite genotype value in the prediction panel");
    return NGP_OK;
}

int end_prediction(ngp_handle *h) {
    REQUIRE(h->pred_open && h->pm && h->pm->pred, NGP_ERR_STATE, "no open prediction panel (ngp_begin_prediction_panel)");
    HCHK(hipStreamSynchronize(h->stream));
    h->pm->pred->done = true;
    h->pred_open = false;
    return ensure_prediction(h, false);
}

// ---- PLINK .bed columns (ngp_bed.h; DESIGN.md section 2, "PLINK .bed panels") ----
// Packed SNP-major columns [col0, col0 + ncol) of the open training panel (pred == false) or of the open prediction panel: staged as
// they are in the file in chunks of whole columns (256 MiB), counted, decoded, gathered by rows[] and tiled on the device.  Every
// argument is checked here, before any launch: an index of rows[] outside the file never reaches a kernel.
int bed_columns(ngp_handle *h, bool pred, int64_t col0, const uint8_t *packed, int64_t ncol, int64_t stride, int64_t n_file, const int64_t *rows,
                int allele, int missing, int centre, int64_t *counts) {
    int rc;
    if ((rc = enter(h, pred))) return rc;
    if (pred) REQUIRE(h->pred_open && h->pm && h->pm->pred, NGP_ERR_STATE, "ngp_prediction_columns_bed needs an open prediction panel (ngp_begin_prediction_panel)");
    else REQUIRE(h->panel_open && h->pm, NGP_ERR_STATE, "ngp_panel_columns_bed needs an open panel (ngp_begin_panel)");
    const int64_t N = pred ? h->pm->pred->Np : h->N;
    const int R = pred ? (int)h->pm->pred->R : (int)h->plan.R, S = pred ? (int)h->pm->pred->S : (int)h->plan.S;
    REQUIRE(packed != nullptr, NGP_ERR_ARG, "null pointer to the packed .bed columns");
    REQUIRE(n_file >= 1 && n_file <= ((int64_t)1 << 40), NGP_ERR_ARG, ".bed columns: n_file must be at least 1");
    const int64_t colbytes = (n_file + 3) / 4;
    REQUIRE(stride >= colbytes, NGP_ERR_ARG, ".bed columns: stride " + std::to_string(stride) + " is smaller than ceil(n_file / 4) = " + std::to_string(colbytes));
    REQUIRE(col0 >= 0 && ncol > 0 && col0 + ncol <= h->P, NGP_ERR_ARG, "column range outside the panel");
    REQUIRE(rows != nullptr || n_file == N, NGP_ERR_ARG,
            ".bed columns without a row map: the file holds " + std::to_string(n_file) + " samples, the panel " + std::to_string(N) + " rows");
    if (rows)
        for (int64_t i = 0; i < N; i++)
            REQUIRE(rows[i] >= 0 && rows[i] < n_file, NGP_ERR_ARG,
                    ".bed row map: rows[" + std::to_string(i) + "] = " + std::to_string(rows[i]) + " is outside the file's " + std::to_string(n_file) + " samples");
    REQUIRE(allele == 1 || allele == 2, NGP_ERR_ARG, ".bed columns: allele must be 1 (count A1) or 2 (count A2)");
    REQUIRE(missing == NGP_BED_MISSING_ERROR || missing == NGP_BED_MISSING_MEAN || missing == NGP_BED_MISSING_ROUND, NGP_ERR_ARG,
            ".bed columns: unknown missing-call policy " + std::to_string(missing));
    REQUIRE(!(missing == NGP_BED_MISSING_MEAN && h->req.storage == 1), NGP_ERR_ARG,
            ".bed columns: NGP_BED_MISSING_MEAN needs fp32 storage (byte tiles hold genotype codes: NGP_BED_MISSING_ROUND)");
    REQUIRE(!(pred && missing == NGP_BED_MISSING_MEAN && centre == 0), NGP_ERR_ARG,
            ".bed prediction columns: NGP_BED_MISSING_MEAN writes the training mean, which needs centre != 0");
    const int64_t L = (int64_t)R * S;
    const unsigned lut = allele == 1 ? NGP_BED_LUT_A1 : NGP_BED_LUT_A2;
    const int64_t cchunk = std::max<int64_t>(1, std::min<int64_t>(ncol, staging_bytes(h, (int64_t)256 << 20) / stride));
    DevArray<uint8_t> d_g;
    DevArray<long long> d_rows, d_cnt;
    DevArray<double> d_vm;
    if (d_g.alloc_raw((size_t)cchunk * (size_t)stride) != hipSuccess) return fail(h, NGP_ERR_NOMEM, "staging buffer");
    if ((rc = d_cnt.alloc(h, (size_t)cchunk * 4)) || (rc = d_vm.alloc(h, (size_t)cchunk))) return rc;
    if (rows) {  // the row map goes up once per call
        if (d_rows.alloc_raw((size_t)N) != hipSuccess) return fail(h, NGP_ERR_NOMEM, ".bed row map");
        HCHK(hipMemcpyAsync(d_rows, rows, (size_t)N * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    }
    const bool want_cnt = counts != nullptr || missing == NGP_BED_MISSING_ERROR;
    std::vector<long long> cnt(want_cnt ? (size_t)cchunk * 4 : 0);
    for (int64_t c0 = 0; c0 < ncol; c0 += cchunk) {
        const int64_t nc = std::min<int64_t>(cchunk, ncol - c0), j0 = col0 + c0;
        // the last column may end ceil(n_file / 4) bytes in: nc - 1 full strides + one column's bytes
        HCHK(hipMemcpyAsync(d_g, packed + (size_t)c0 * (size_t)stride, (size_t)(nc - 1) * (size_t)stride + (size_t)colbytes, hipMemcpyHostToDevice, h->stream));
        double *d_mu = pred ? h->pm->pred->mean + j0 : h->pm->mean + j0;
        const double *d_train = pred ? h->pm->mean + j0 : nullptr;
        hipLaunchKernelGGL(k_bed_stats, dim3((unsigned)nc), dim3(256), 0, h->stream, (const uint8_t *)d_g, (long long)stride, (const long long *)d_rows.get(),
                           (long long)N, lut, missing, centre, d_train, d_cnt.get(), d_mu, d_vm.get());
        if (want_cnt) {
            HCHK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)nc * 4 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
            HCHK(hipStreamSynchronize(h->stream));
            if (counts)
                for (int64_t k = 0; k < nc * 4; k++) counts[(size_t)c0 * 4 + (size_t)k] = (int64_t)cnt[(size_t)k];
            if (missing == NGP_BED_MISSING_ERROR)
                for (int64_t c = 0; c < nc; c++)
                    REQUIRE(cnt[(size_t)c * 4 + 3] == 0, NGP_ERR_ARG,
                            "column " + std::to_string(j0 + c) + " holds " + std::to_string(cnt[(size_t)c * 4 + 3]) + " missing calls");
        }
        if (h->req.storage == 1)
            hipLaunchKernelGGL(k_bed_fill8, dim3((unsigned)((L / 16 + 255) / 256), (unsigned)nc), dim3(256), 0, h->stream,
                               pred ? (uint8_t *)h->pm->pred->tiles.get() : (uint8_t *)h->pm->tiles.get(), (const uint8_t *)d_g, (long long)stride,
                               (const long long *)d_rows.get(), (long long)N, lut, (long long)j0, R, S, (const double *)d_vm.get());
        else  // residual weights never scale prediction rows
            hipLaunchKernelGGL(k_bed_fill, dim3((unsigned)((L / 4 + 255) / 256), (unsigned)nc), dim3(256), 0, h->stream,
                               pred ? h->pm->pred->tiles.get() : h->pm->tiles.get(), (const uint8_t *)d_g, (long long)stride, (const long long *)d_rows.get(),
                               (long long)N, lut, (long long)j0, R, S, (const double *)d_mu, (const double *)d_vm.get(),
                               pred ? (const double *)nullptr : (const double *)h->cm.d_rs);
        HCHK(hipGetLastError());
        HCHK(hipStreamSynchronize(h->stream));  // the staging buffer is reused by the next chunk
    }
    return NGP_OK;
}

// the chain's prediction arrays, checked against the caller's shape
int prediction_shape(ngp_handle *h, int64_t rows, int64_t Np) {
    int rc;
    if ((rc = ensure_prediction(h, false))) return rc;
    REQUIRE(predicts(h), NGP_ERR_STATE, "no prediction: a finished prediction panel (ngp_end_prediction_panel) and at least one marker set are needed");
    REQUIRE(rows == h->cm.pred_rows && Np == h->pm->pred->Np, NGP_ERR_ARG,
            "prediction arrays are [nsets + 1][Np] = [" + std::to_string(h->cm.pred_rows) + "][" + std::to_string(h->pm->pred->Np) + "]");
    HCHK(hipStreamSynchronize(h->stream));
    return NGP_OK;
}
}  // namespace

extern "C" {

int32_t ngp_begin_prediction_panel(ngp_handle *h, int64_t Np) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    return begin_prediction(h, Np);
    NGP_CATCH(h)
}
int32_t ngp_prediction_columns_f64(ngp_handle *h, int64_t col0, const double *M, int64_t ncol, int64_t ld, int32_t centre) {
    NGP_TRY
    return prediction_columns<double>(h, col0, M, ncol, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_prediction_columns_f32(ngp_handle *h, int64_t col0, const float *M, int64_t ncol, int64_t ld, int32_t centre) {
    NGP_TRY
    return prediction_columns<float>(h, col0, M, ncol, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_prediction_columns_u8(ngp_handle *h, int64_t col0, const uint8_t *G, int64_t ncol, int64_t ld, int32_t centre) {
    NGP_TRY
    return prediction_columns<uint8_t>(h, col0, G, ncol, ld, centre);
    NGP_CATCH(h)
}
int32_t ngp_panel_columns_bed(ngp_handle *h, int64_t col0, const uint8_t *packed, int64_t ncol, int64_t stride, int64_t n_file,
                              const int64_t *rows, int32_t allele, int32_t missing, int32_t centre, int64_t *counts) {
    NGP_TRY
    return bed_columns(h, false, col0, packed, ncol, stride, n_file, rows, allele, missing, centre, counts);
    NGP_CATCH(h)
}
int32_t ngp_prediction_columns_bed(ngp_handle *h, int64_t col0, const uint8_t *packed, int64_t ncol, int64_t stride, int64_t n_file,
                                   const int64_t *rows, int32_t allele, int32_t missing, int32_t centre, int64_t *counts) {
    NGP_TRY
    return bed_columns(h, true, col0, packed, ncol, stride, n_file, rows, allele, missing, centre, counts);
    NGP_CATCH(h)
}
int32_t ngp_end_prediction_panel(ngp_handle *h) {
    NGP_TRY
    int rc;
    if ((rc = enter(h, true))) return rc;
    return end_prediction(h);
    NGP_CATCH(h)
}

int32_t ngp_load_prediction_file(ngp_handle *h, const char *path, int32_t centre) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(path != nullptr, NGP_ERR_ARG, "null path");
    REQUIRE(h->pm && !h->panel_open, NGP_ERR_STATE, "a prediction panel needs a finished training panel (ngp_set_panel_* / ngp_end_panel)");
    File f(std::fopen(path, "rb"));
    REQUIRE(f != nullptr, NGP_ERR_ARG, std::string("cannot open panel file ") + path);
    PanelHeader hd;
    if (std::fread(&hd, sizeof hd, 1, f.get()) != 1 || std::memcmp(hd.magic, "NGPPNL01", 8) != 0 || hd.N <= 0 || hd.P <= 0 || (hd.bits != 8 && hd.bits != 2))
        return fail(h, NGP_ERR_ARG, std::string("not a panel file (magic NGPPNL01, bits 8 or 2): ") + path);
    REQUIRE(hd.P == h->P, NGP_ERR_ARG, "the prediction file holds " + std::to_string(hd.P) + " columns, the training panel " + std::to_string(h->P));
    const int64_t N = hd.N, P = hd.P;
    if ((rc = begin_prediction(h, N))) return rc;
    // whole columns through a host buffer of about 64 MiB; two-bit columns are unpacked on the host
    const int64_t colbytes = (hd.bits == 8) ? N : (N + 3) / 4;
    const int64_t cchunk = std::max<int64_t>(1, std::min<int64_t>(P, staging_bytes(h, (int64_t)64 << 20) / N));
    std::vector<uint8_t> buf((size_t)cchunk * (size_t)N), packed((hd.bits == 2) ? (size_t)colbytes : 0);
    std::string why;
    rc = NGP_OK;
    for (int64_t c0 = 0; c0 < P && why.empty() && rc == NGP_OK; c0 += cchunk) {
        const int64_t nc = std::min<int64_t>(cchunk, P - c0);
        for (int64_t jc = 0; jc < nc && why.empty(); jc++) {
            uint8_t *dst = buf.data() + (size_t)jc * N;
            if (hd.bits == 8) {
                if (std::fread(dst, 1, (size_t)N, f.get()) != (size_t)N) why = "panel file truncated";
            } else {
                if (std::fread(packed.data(), 1, packed.size(), f.get()) != packed.size()) { why = "panel file truncated"; break; }
                for (int64_t i = 0; i < N; i++) {
                    const uint8_t g = (uint8_t)((packed[(size_t)i >> 2] >> (2 * (i & 3))) & 3u);
                    if (g == 3) { why = "panel file holds a missing genotype (code 3): impute before loading"; break; }
                    dst[i] = g;
                }
            }
        }
        if (why.empty()) rc = prediction_columns<uint8_t>(h, c0, buf.data(), nc, N, centre);
    }
    if (!why.empty()) { drop_prediction(h); return fail(h, NGP_ERR_ARG, why); }
    if (rc) { drop_prediction(h); return rc; }
    return end_prediction(h);
    NGP_CATCH(h)
}

int32_t ngp_get_prediction_layout(ngp_handle *h, int64_t *Np, int64_t *R, int64_t *S, int64_t *chunk_cols, int64_t *rows) {
    NGP_TRY
    int rc;
    if ((rc = enter(h, true))) return rc;
    REQUIRE(h->pm && h->pm->pred, NGP_ERR_STATE, "no prediction panel");
    if (Np) *Np = h->pm->pred->Np;
    if (R) *R = h->pm->pred->R;
    if (S) *S = h->pm->pred->S;
    if (chunk_cols) *chunk_cols = (int64_t)NGP_PRED_CB * NGP_BLK;
    if (rows) *rows = h->sets.empty() ? 0 : (int64_t)h->sets.size() + 1;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_prediction(ngp_handle *h, double *sum, double *sum2, int64_t rows, int64_t Np, int64_t *nKept) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = prediction_shape(h, rows, Np))) return rc;
    const size_t bytes = (size_t)rows * (size_t)Np * sizeof(double);
    if (sum) HCHK(hipMemcpy(sum, h->cm.d_pred_sum, bytes, hipMemcpyDeviceToHost));
    if (sum2) HCHK(hipMemcpy(sum2, h->cm.d_pred_sum2, bytes, hipMemcpyDeviceToHost));
    if (nKept) {
        DScal sc;
        HCHK(hipMemcpy(&sc, h->cm.d_scal, sizeof(DScal), hipMemcpyDeviceToHost));
        *nKept = (int64_t)sc.nKept;
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_prediction(ngp_handle *h, const double *sum, const double *sum2, int64_t rows, int64_t Np) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(sum && sum2, NGP_ERR_ARG, "null prediction sums");
    if ((rc = prediction_shape(h, rows, Np))) return rc;
    const size_t bytes = (size_t)rows * (size_t)Np * sizeof(double);
    HCHK(hipMemcpy(h->cm.d_pred_sum, sum, bytes, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(h->cm.d_pred_sum2, sum2, bytes, hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_prediction_last(ngp_handle *h, double *out, int64_t rows, int64_t Np) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(out != nullptr, NGP_ERR_ARG, "null output");
    if ((rc = prediction_shape(h, rows, Np))) return rc;
    HCHK(hipMemcpy(out, h->cm.d_pred_last, (size_t)rows * (size_t)Np * sizeof(double), hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_prediction_stats(ngp_handle *h, int64_t *launches, int64_t *chains_served) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (launches) *launches = h->cm.pred_launches;
    if (chains_served) *chains_served = h->cm.pred_served;
    return NGP_OK;
    NGP_CATCH(h)
}

/* ---- genomic variance (ngp_genvar.h; DESIGN.md section 2, "Genomic variance") ---- */

int32_t ngp_set_variance_windows(ngp_handle *h, int32_t set_id, const int64_t *start, const int64_t *stop, int64_t nwin) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && !h->panel_open && !h->records_only, NGP_ERR_STATE, "variance windows need a finished panel and a marker set");
    REQUIRE(set_id >= 0 && (size_t)set_id < h->sets.size(), NGP_ERR_ARG, "variance windows: no marker set " + std::to_string(set_id));
    REQUIRE(nwin >= 0 && (nwin == 0 || (start && stop)), NGP_ERR_ARG, "variance windows: null arrays");
    const int64_t ncol = h->sets[(size_t)set_id].ncol;
    std::vector<int64_t> w;
    int64_t at = 0;
    for (int64_t k = 0; k < nwin; k++) {
        REQUIRE(start[k] >= at && stop[k] > start[k] && stop[k] <= ncol, NGP_ERR_ARG,
                "variance windows must be ascending, disjoint, non-empty and inside the set's " + std::to_string(ncol) + " columns (window " + std::to_string(k) + ")");
        w.push_back(start[k]); w.push_back(stop[k]);
        at = stop[k];
    }
    GenVar &g = h->cm.gv;
    g.win.resize(h->sets.size());
    g.win[(size_t)set_id] = std::move(w);
    g.built = false;  // (the sums go with the tables)
    return ensure_genvar(h, false);
    NGP_CATCH(h)
}

int32_t ngp_enable_genomic_variance(ngp_handle *h, int32_t on, double threshold, int64_t trace_rows) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    GenVar &g = h->cm.gv;
    if (!on) { g.on = false; g.built = false; return NGP_OK; }
    REQUIRE(h->pm && !h->panel_open, NGP_ERR_STATE, "genomic variance needs a finished training panel (ngp_set_panel_* / ngp_end_panel)");
    REQUIRE(!h->records_only, NGP_ERR_STATE, "a records-only (GBLUP) handle has no marker panel whose variance could be formed");
    REQUIRE(h->h_rw.empty(), NGP_ERR_STATE, "genomic variance with residual weights is not supported: the tiles hold row-scaled values whose variance is not var(X beta)");
    REQUIRE(h->N >= 2, NGP_ERR_STATE, "genomic variance needs at least two individuals");
    REQUIRE(h->N <= NGP_GV_MAXN, NGP_ERR_STATE, "genomic variance: more than 2^18 individuals would leave the head-room of the 64-bit fixed-point sums");
    REQUIRE(threshold >= 0.0 && threshold <= 1.0, NGP_ERR_ARG, "genomic variance: the threshold is a share of the variance, in [0, 1]");
    REQUIRE(trace_rows >= 0 && trace_rows <= ((int64_t)1 << 32), NGP_ERR_ARG, "genomic variance: trace_rows must be >= 0");
    REQUIRE(genvar_lds_bytes(NGP_GV_MAXK, h->req.storage == 1) <= NGP_LDS_MAX, NGP_ERR_STATE, "genomic variance: LDS of the pass exceeds 160 KiB");
    HCHK(genvar_prepare());
    g.on = true; g.thr = threshold; g.trace_rows = trace_rows;
    g.built = false;
    return ensure_genvar(h, false);
    NGP_CATCH(h)
}

int32_t ngp_get_genomic_variance_layout(ngp_handle *h, int64_t *nslots, int64_t *nwin_total, int64_t *nsets, int64_t *traced, int64_t *trace_dropped) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = ensure_genvar(h, false))) return rc;
    REQUIRE(gv_active(h), NGP_ERR_STATE, "no genomic variance: ngp_enable_genomic_variance and at least one marker set are needed");
    const GenVar &g = h->cm.gv;
    long long cnt[2] = {0, 0};
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(cnt, g.d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
    if (nslots) *nslots = g.nslots;
    if (nwin_total) *nwin_total = g.nwin;
    if (nsets) *nsets = (int64_t)h->sets.size();
    if (traced) *traced = std::min<int64_t>(cnt[0], g.trace_rows);
    if (trace_dropped) *trace_dropped = cnt[0] - std::min<int64_t>(cnt[0], g.trace_rows);
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_genomic_variance(ngp_handle *h, double *sumV, double *sumV2, double *sumQ, double *sumQ2, double *count, double *last, int64_t nslots,
                                 double *ratio, int64_t *nKept) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = ensure_genvar(h, false))) return rc;
    REQUIRE(gv_active(h), NGP_ERR_STATE, "no genomic variance: ngp_enable_genomic_variance and at least one marker set are needed");
    const GenVar &g = h->cm.gv;
    REQUIRE(nslots == g.nslots, NGP_ERR_ARG, "genomic variance arrays hold nslots = " + std::to_string(g.nslots) + " entries");
    HCHK(hipStreamSynchronize(h->stream));
    double *out[6] = {sumV, sumV2, sumQ, sumQ2, count, last};
    for (int a = 0; a < 6; a++)
        if (out[a]) HCHK(hipMemcpy(out[a], g.d_acc.get() + (size_t)a * g.nslots, (size_t)g.nslots * sizeof(double), hipMemcpyDeviceToHost));
    if (ratio) HCHK(hipMemcpy(ratio, g.d_acc.get() + (size_t)6 * g.nslots, 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (nKept) {
        long long cnt[2] = {0, 0};
        HCHK(hipMemcpy(cnt, g.d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
        *nKept = (int64_t)cnt[0];
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_genomic_variance(ngp_handle *h, const double *sumV, const double *sumV2, const double *sumQ, const double *sumQ2, const double *count,
                                 const double *last, int64_t nslots, const double *ratio, int64_t nKept) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = ensure_genvar(h, false))) return rc;
    REQUIRE(gv_active(h), NGP_ERR_STATE, "no genomic variance: ngp_enable_genomic_variance and at least one marker set are needed");
    GenVar &g = h->cm.gv;
    REQUIRE(nslots == g.nslots, NGP_ERR_ARG, "genomic variance arrays hold nslots = " + std::to_string(g.nslots) + " entries");
    REQUIRE(nKept >= 0, NGP_ERR_ARG, "genomic variance: nKept must be >= 0");
    HCHK(hipStreamSynchronize(h->stream));
    const double *in[6] = {sumV, sumV2, sumQ, sumQ2, count, last};
    for (int a = 0; a < 6; a++)
        if (in[a]) HCHK(hipMemcpy(g.d_acc.get() + (size_t)a * g.nslots, in[a], (size_t)g.nslots * sizeof(double), hipMemcpyHostToDevice));
    if (ratio) HCHK(hipMemcpy(g.d_acc.get() + (size_t)6 * g.nslots, ratio, 2 * sizeof(double), hipMemcpyHostToDevice));
    const long long cnt[2] = {(long long)nKept, (long long)nKept};
    HCHK(hipMemcpy(g.d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_genomic_variance_trace(ngp_handle *h, double *V, double *ratio, int64_t rows, int64_t nslots) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if ((rc = ensure_genvar(h, false))) return rc;
    REQUIRE(gv_active(h), NGP_ERR_STATE, "no genomic variance: ngp_enable_genomic_variance and at least one marker set are needed");
    const GenVar &g = h->cm.gv;
    REQUIRE(nslots == g.nslots, NGP_ERR_ARG, "genomic variance arrays hold nslots = " + std::to_string(g.nslots) + " entries");
    long long cnt[2] = {0, 0};
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(cnt, g.d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
    REQUIRE(rows >= 0 && rows <= std::min<int64_t>(cnt[0], g.trace_rows), NGP_ERR_ARG,
            "genomic variance trace: " + std::to_string(std::min<int64_t>(cnt[0], g.trace_rows)) + " rows are stored");
    if (rows == 0) return NGP_OK;
    std::vector<double> t((size_t)rows * (size_t)(nslots + 1));
    HCHK(hipMemcpy(t.data(), g.d_trace, t.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < rows; r++) {
        if (V) std::memcpy(V + (size_t)r * nslots, t.data() + (size_t)r * (nslots + 1), (size_t)nslots * sizeof(double));
        if (ratio) ratio[r] = t[(size_t)r * (nslots + 1) + nslots];
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_genomic_variance_stats(ngp_handle *h, int64_t *launches, int64_t *chains_served) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (launches) *launches = h->cm.gv.launches;
    if (chains_served) *chains_served = h->cm.gv.served;
    return NGP_OK;
    NGP_CATCH(h)
}

/* ---- convergence diagnostics (ngp_diag.h; DESIGN.md section 2, "Convergence diagnostics") ---- */

int32_t ngp_enable_diagnostics(ngp_handle *h, int32_t on, int32_t lags, int64_t split) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    Diag &g = h->cm.dg;
    if (!on) { HCHK(hipStreamSynchronize(h->stream)); h->cm.dg = Diag(); return NGP_OK; }
    REQUIRE(h->pm && !h->panel_open, NGP_ERR_STATE, "convergence diagnostics need a model: a finished panel (ngp_set_panel_* / ngp_end_panel) or ngp_set_records");
    REQUIRE(lags >= 2 && lags <= NGP_DIAG_MAXL && lags % 2 == 0, NGP_ERR_ARG, "convergence diagnostics: lags must be even, 2 .. 256");
    REQUIRE(split >= 0, NGP_ERR_ARG, "convergence diagnostics: split must be >= 0");
    HCHK(hipStreamSynchronize(h->stream));
    const int64_t launches = g.launches;
    h->cm.dg = Diag();
    g.on = true; g.L = lags; g.split = split; g.launches = launches;
    return ensure_diag(h, true);
    NGP_CATCH(h)
}

int32_t ngp_get_diagnostics_layout(ngp_handle *h, int64_t *D, int32_t *lags, int64_t *split, int64_t *n, int64_t *state_words) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->cm.dg.on, NGP_ERR_STATE, "no convergence diagnostics: ngp_enable_diagnostics is needed");
    if ((rc = ensure_diag(h, false))) return rc;
    const Diag &g = h->cm.dg;
    if (D) *D = g.D;
    if (lags) *lags = g.L;
    if (split) *split = g.split;
    if (n) *n = g.n;
    if (state_words) *state_words = (int64_t)DiagRows::rows(g.L) * g.D;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_diagnostics(ngp_handle *h, double *mean, double *var, double *ess, double *mcse, double *truncated, double *half_n, double *half_mean,
                            double *half_var, int64_t D, int64_t *n) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->cm.dg.on, NGP_ERR_STATE, "no convergence diagnostics: ngp_enable_diagnostics is needed");
    if ((rc = ensure_diag(h, false))) return rc;
    const Diag &g = h->cm.dg;
    REQUIRE(D == g.D, NGP_ERR_ARG, "convergence diagnostics arrays hold D = " + std::to_string(g.D) + " entries");
    if (n) *n = g.n;
    if (g.n == 0) return NGP_OK;
    DevArray<double> d_out;
    if ((rc = d_out.alloc(h, (size_t)NGP_DIAG_OUT * (size_t)D))) return rc;
    hipLaunchKernelGGL(k_diag_finalise, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, h->stream, (const double *)g.d_st.get(), (long long)g.Dp, (long long)D, g.L,
                       (long long)g.n, (long long)g.split, d_out.get());
    HCHK(hipStreamSynchronize(h->stream));
    double *out[5] = {mean, var, ess, mcse, truncated};
    for (int a = 0; a < 5; a++)
        if (out[a]) HCHK(hipMemcpy(out[a], d_out.get() + (size_t)a * D, (size_t)D * sizeof(double), hipMemcpyDeviceToHost));
    if (half_mean) HCHK(hipMemcpy(half_mean, d_out.get() + (size_t)5 * D, (size_t)2 * D * sizeof(double), hipMemcpyDeviceToHost));
    if (half_var) HCHK(hipMemcpy(half_var, d_out.get() + (size_t)7 * D, (size_t)2 * D * sizeof(double), hipMemcpyDeviceToHost));
    if (half_n) { half_n[0] = (double)std::min<int64_t>(g.n, g.split); half_n[1] = (double)(g.n - std::min<int64_t>(g.n, g.split)); }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_diagnostics_state(ngp_handle *h, double *state, int64_t words, int64_t *n) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->cm.dg.on, NGP_ERR_STATE, "no convergence diagnostics: ngp_enable_diagnostics is needed");
    if ((rc = ensure_diag(h, false))) return rc;
    const Diag &g = h->cm.dg;
    const int64_t rows = (int64_t)DiagRows::rows(g.L);
    REQUIRE(state && words == rows * g.D, NGP_ERR_ARG, "convergence diagnostics state holds (3 lags + 5) D = " + std::to_string(rows * g.D) + " words");
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy2D(state, (size_t)g.D * 8, g.d_st.get(), (size_t)g.Dp * 8, (size_t)g.D * 8, (size_t)rows, hipMemcpyDeviceToHost));
    if (n) *n = g.n;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_diagnostics_state(ngp_handle *h, const double *state, int64_t words, int64_t n) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->cm.dg.on, NGP_ERR_STATE, "no convergence diagnostics: ngp_enable_diagnostics is needed");
    if ((rc = ensure_diag(h, false))) return rc;
    Diag &g = h->cm.dg;
    const int64_t rows = (int64_t)DiagRows::rows(g.L);
    REQUIRE(state && words == rows * g.D, NGP_ERR_ARG, "convergence diagnostics state holds (3 lags + 5) D = " + std::to_string(rows * g.D) + " words");
    REQUIRE(n >= 0, NGP_ERR_ARG, "convergence diagnostics: n must be >= 0");
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy2D(g.d_st.get(), (size_t)g.Dp * 8, state, (size_t)g.D * 8, (size_t)g.D * 8, (size_t)rows, hipMemcpyHostToDevice));
    g.n = n; g.fixed = true;
    return NGP_OK;
    NGP_CATCH(h)
}

/* Timing hook of the diagnostics (tools/diag_time.py): device events around `reps` full-window updates (k_diag_gather + k_diag_update
 * at draw indices >= lags, on a scratch copy of the chain's state -- the chain's own state and draw count stay what they are) and
 * around `reps` launches of k_diag_finalise over the chain's state; milliseconds per launch.  The finalise leg needs a draw taken
 * (0 otherwise). */
int32_t ngp_debug_time_diagnostics(ngp_handle *h, int32_t reps, double *update_ms, double *finalise_ms) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->cm.dg.on, NGP_ERR_STATE, "no convergence diagnostics: ngp_enable_diagnostics is needed");
    REQUIRE(reps >= 1 && reps <= 1000, NGP_ERR_ARG, "reps: 1 .. 1000");
    if ((rc = ensure_diag(h, false))) return rc;
    const Diag &g = h->cm.dg;
    const size_t words = (size_t)DiagRows::rows(g.L) * (size_t)g.Dp;
    DevArray<double> d_scr, d_out;
    if ((rc = d_scr.alloc(h, words)) || (rc = d_out.alloc(h, (size_t)NGP_DIAG_OUT * (size_t)g.D))) { (void)hipGetLastError(); return rc; }
    HCHK(hipMemcpyAsync(d_scr, g.d_st, words * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    const long long np = (long long)(g.Dp / 2), t0 = std::max<long long>((long long)g.n, (long long)g.L);
    float ms = 0.f;
    for (int leg = 0; leg < 2; leg++) {
        if (leg == 1 && g.n == 0) { if (finalise_ms) *finalise_ms = 0.0; break; }
        for (int r = -1; r < reps; r++) {  // (r = -1: a launch in front of the timed ones)
            if (r == 0) HCHK(hipEventRecord(h->ev0, h->stream));
            if (leg == 0) {
                hipLaunchKernelGGL(k_diag_gather, dim3((unsigned)((g.maxw + 255) / 256), (unsigned)g.segs.size()), dim3(256), 0, h->stream,
                                   (const DiagSeg *)g.d_segs.get(), g.d_x.get(), (const unsigned *)nullptr);
                hipLaunchKernelGGL(k_diag_update, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, (const double2 *)g.d_x.get(), (double2 *)d_scr.get(), np,
                                   g.L, t0 + r + 1, (long long)g.split, (const unsigned *)nullptr);
            } else
                hipLaunchKernelGGL(k_diag_finalise, dim3((unsigned)((g.D + 255) / 256)), dim3(256), 0, h->stream, (const double *)g.d_st.get(), (long long)g.Dp,
                                   (long long)g.D, g.L, (long long)g.n, (long long)g.split, d_out.get());
        }
        HCHK(hipEventRecord(h->ev1, h->stream));
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        if (leg == 0 && update_ms) *update_ms = (double)ms / reps;
        if (leg == 1 && finalise_ms) *finalise_ms = (double)ms / reps;
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_diagnostics_stats(ngp_handle *h, int64_t *launches) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    if (launches) *launches = h->cm.dg.launches;
    return NGP_OK;
    NGP_CATCH(h)
}

/* Held-out records ("Held-out records"; kernels in ngp_holdout.h): m strictly increasing rows whose phenotypes
 * are not read but redrawn from their conditional at the head of every iteration.  Set after the panel (or ngp_set_records /
 * ngp_share_panel: a sharer does not inherit the owner's mask) and before ngp_set_y; NULL, 0 removes the mask. */
int32_t ngp_set_holdout(ngp_handle *h, const int64_t *rows, int64_t m) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set (the hold-out set belongs to the panel's records)");
    REQUIRE(!h->have_y, NGP_ERR_STATE, "ngp_set_holdout: the phenotypes are set already; the hold-out set comes before ngp_set_y");
    REQUIRE(!h->cm.lb.on(), NGP_ERR_STATE, "ngp_set_holdout: this handle has liability traits already; the hold-out set comes before them (they leave its rows out)");
    REQUIRE(m >= 0 && (rows != nullptr || m == 0), NGP_ERR_ARG, "ngp_set_holdout: m >= 0 rows (or NULL and 0 to remove the mask)");
    REQUIRE(m < h->N, NGP_ERR_ARG, "ngp_set_holdout: at least one record must keep its phenotype (m < N)");
    for (int64_t k = 0; k < m; k++)
        REQUIRE(rows[k] >= 0 && rows[k] < h->N && (k == 0 || rows[k] > rows[k - 1]), NGP_ERR_ARG,
                "ngp_set_holdout: rows must be strictly increasing and lie in [0, N)");
    ChainMem &c = h->cm;
    c.ho_rows.clear();
    c.d_ho_rows.reset(); c.d_yaug.reset(); c.d_sum_fit.reset(); c.d_sum_fit2.reset(); c.d_n_fit.reset();
    if (m == 0) return NGP_OK;
    std::vector<long long> r(rows, rows + m);
    DevArray<long long> d_rows;
    DevArray<double> d_yaug, d_s, d_s2, d_n;
    if ((rc = d_rows.alloc(h, (size_t)m)) || (rc = d_yaug.alloc(h, (size_t)m)) || (rc = d_s.alloc(h, (size_t)h->N)) || (rc = d_s2.alloc(h, (size_t)h->N)) ||
        (rc = d_n.alloc(h, (size_t)h->N)))
        return rc;
    HCHK(hipMemcpyAsync(d_rows, r.data(), (size_t)m * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HCHK(hipStreamSynchronize(h->stream));
    c.ho_rows = std::move(r);
    c.d_ho_rows = std::move(d_rows); c.d_yaug = std::move(d_yaug); c.d_sum_fit = std::move(d_s); c.d_sum_fit2 = std::move(d_s2); c.d_n_fit = std::move(d_n);
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_holdout_layout(ngp_handle *h, int64_t *m) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    if (m) *m = (int64_t)h->cm.ho_rows.size();
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_get_holdout(ngp_handle *h, int64_t *rows, double *yaug, double *sum_fit, double *sum_fit2, double *n_fit, int64_t m, int64_t N) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && !h->cm.ho_rows.empty(), NGP_ERR_STATE, "no hold-out set on this handle (ngp_set_holdout)");
    REQUIRE(m == (int64_t)h->cm.ho_rows.size() && N == h->N, NGP_ERR_ARG, "hold-out buffers must hold m and N entries (ngp_get_holdout_layout)");
    REQUIRE(h->have_y || !(yaug || sum_fit || sum_fit2 || n_fit), NGP_ERR_STATE, "y not set: the hold-out state does not exist yet");
    HCHK(hipStreamSynchronize(h->stream));
    if (rows) for (int64_t k = 0; k < m; k++) rows[k] = (int64_t)h->cm.ho_rows[(size_t)k];
    const size_t N8 = (size_t)N * sizeof(double);
    if (yaug) HCHK(hipMemcpy(yaug, h->cm.d_yaug, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (sum_fit) HCHK(hipMemcpy(sum_fit, h->cm.d_sum_fit, N8, hipMemcpyDeviceToHost));
    if (sum_fit2) HCHK(hipMemcpy(sum_fit2, h->cm.d_sum_fit2, N8, hipMemcpyDeviceToHost));
    if (n_fit) HCHK(hipMemcpy(n_fit, h->cm.d_n_fit, N8, hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_holdout_state(ngp_handle *h, const double *yaug, const double *sum_fit, const double *sum_fit2, const double *n_fit, int64_t m, int64_t N) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm && !h->cm.ho_rows.empty(), NGP_ERR_STATE, "no hold-out set on this handle (ngp_set_holdout)");
    REQUIRE(h->have_y, NGP_ERR_STATE, "y not set (ngp_set_y starts the hold-out state, this call replaces it)");
    REQUIRE(m == (int64_t)h->cm.ho_rows.size() && N == h->N, NGP_ERR_ARG, "hold-out buffers must hold m and N entries (ngp_get_holdout_layout)");
    if (yaug) for (int64_t k = 0; k < m; k++) REQUIRE(std::isfinite(yaug[k]), NGP_ERR_ARG, "non-finite augmented phenotype");
    for (const double *a : {sum_fit, sum_fit2, n_fit})
        if (a) for (int64_t i = 0; i < N; i++) REQUIRE(std::isfinite(a[i]), NGP_ERR_ARG, "non-finite hold-out sum");
    HCHK(hipStreamSynchronize(h->stream));
    const size_t N8 = (size_t)N * sizeof(double);
    if (yaug) HCHK(hipMemcpy(h->cm.d_yaug, yaug, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
    if (sum_fit) HCHK(hipMemcpy(h->cm.d_sum_fit, sum_fit, N8, hipMemcpyHostToDevice));
    if (sum_fit2) HCHK(hipMemcpy(h->cm.d_sum_fit2, sum_fit2, N8, hipMemcpyHostToDevice));
    if (n_fit) HCHK(hipMemcpy(h->cm.d_n_fit, n_fit, N8, hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Liability traits ("Liability traits"; kernels in ngp_liability.h).  A record with a liability keeps its row in
 * the panel; its latent value is redrawn from a truncated normal at the head of every iteration.  Both setters come after the panel
 * (or ngp_set_records / ngp_share_panel) and the hold-out mask and before ngp_set_y; they exclude one another; NULL, 0 removes either. */
namespace {
void clear_liabilities(ngp_handle *h) {
    if (h->cm.lb.C > 0) h->fix_varE = 0.0;  // (the classes had fixed it at 1)
    h->cm.lb = Liab();
}
// the device side of a Liab whose host side is filled
int commit_liabilities(ngp_handle *h, Liab &n) {
    int rc;
    const size_t m = n.rows.size();
    if ((rc = ensure_tn_fall(h))) return rc;
    if ((rc = n.d_rows.alloc(h, m)) || (rc = n.d_liab.alloc(h, m))) return rc;
    HCHK(hipMemcpyAsync(n.d_rows, n.rows.data(), m * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    if (n.C >= 2) {
        if ((rc = n.d_cls.alloc(h, m)) || (rc = n.d_thr.alloc(h, 3 * ((size_t)n.C + 1)))) return rc;
        HCHK(hipMemcpyAsync(n.d_cls, n.cls.data(), m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    } else {
        if ((rc = n.d_lo.alloc(h, m)) || (rc = n.d_hi.alloc(h, m))) return rc;
        HCHK(hipMemcpyAsync(n.d_lo, n.lo.data(), m * 8, hipMemcpyHostToDevice, h->stream));
        HCHK(hipMemcpyAsync(n.d_hi, n.hi.data(), m * 8, hipMemcpyHostToDevice, h->stream));
    }
    HCHK(hipStreamSynchronize(h->stream));
    n.digest = liab_digest(n);
    h->cm.lb = std::move(n);
    return NGP_OK;
}
}  // namespace

int32_t ngp_fix_residual_variance(ngp_handle *h, double v) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(std::isfinite(v) && v >= 0.0, NGP_ERR_ARG, "ngp_fix_residual_variance: v > 0 holds varE at v, v = 0 samples it");
    REQUIRE(h->cm.lb.C == 0 || v == 1.0, NGP_ERR_ARG, "ngp_fix_residual_variance: liability classes live on the probit scale, varE = 1");
    h->fix_varE = v;
    if (v > 0.0 && h->pm && h->have_y) {
        hipLaunchKernelGGL(k_set_varE, dim3(1), dim3(1), 0, h->stream, h->cm.d_scal, v);
        HCHK(hipStreamSynchronize(h->stream));
    }
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_liability_classes(ngp_handle *h, const int32_t *cls, int32_t C) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set (the classes belong to the panel's records)");
    REQUIRE(!h->have_y, NGP_ERR_STATE, "ngp_set_liability_classes: the phenotypes are set already; the classes come before ngp_set_y");
    if (cls == nullptr && C == 0) {
        if (h->cm.lb.C > 0) clear_liabilities(h);
        return NGP_OK;
    }
    REQUIRE(h->cm.lb.C > 0 || !h->cm.lb.on(), NGP_ERR_STATE, "ngp_set_liability_classes: this handle has liability bounds (ngp_set_liability_bounds); remove them first");
    REQUIRE(cls != nullptr && C >= 2 && C <= NGP_LIAB_MAXC, NGP_ERR_ARG, "ngp_set_liability_classes: N classes in 1..C with 2 <= C <= 8 (or NULL and 0 to remove them)");
    REQUIRE(h->fix_varE == 0.0 || h->fix_varE == 1.0, NGP_ERR_ARG, "ngp_set_liability_classes: the residual variance is fixed at a value other than 1 (ngp_fix_residual_variance)");
    Liab n;
    n.C = C;
    const std::vector<long long> &ho = h->cm.ho_rows;
    std::vector<long long> cnt((size_t)C + 1, 0);
    size_t kh = 0;
    for (int64_t i = 0; i < h->N; i++) {
        if (kh < ho.size() && ho[kh] == i) { kh++; continue; }  // (entries of held-out rows are not read)
        REQUIRE(cls[i] >= 1 && cls[i] <= C, NGP_ERR_ARG, "ngp_set_liability_classes: a class outside 1..C");
        n.rows.push_back(i); n.cls.push_back(cls[i]); cnt[(size_t)cls[i]] += 1;
    }
    for (int c = 1; c <= C; c++) REQUIRE(cnt[(size_t)c] > 0, NGP_ERR_ARG, "ngp_set_liability_classes: every class needs at least one record that is not held out");
    if ((rc = commit_liabilities(h, n))) return rc;
    h->fix_varE = 1.0;
    return NGP_OK;
    NGP_CATCH(h)
}

int32_t ngp_set_liability_bounds(ngp_handle *h, const int64_t *rows, const double *lo, const double *hi, int64_t m) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set (the bounds belong to the panel's records)");
    REQUIRE(!h->have_y, NGP_ERR_STATE, "ngp_set_liability_bounds: the phenotypes are set already; the bounds come before ngp_set_y");
    if (rows == nullptr && m == 0) {
        if (h->cm.lb.C == 0) clear_liabilities(h);
        return NGP_OK;
    }
    REQUIRE(h->cm.lb.C == 0, NGP_ERR_STATE, "ngp_set_liability_bounds: this handle has liability classes (ngp_set_liability_classes); remove them first");
    REQUIRE(rows && lo && hi && m > 0, NGP_ERR_ARG, "ngp_set_liability_bounds: m > 0 rows with their bounds (or NULL and 0 to remove them)");
    const std::vector<long long> &ho = h->cm.ho_rows;
    for (int64_t k = 0; k < m; k++) {
        REQUIRE(rows[k] >= 0 && rows[k] < h->N && (k == 0 || rows[k] > rows[k - 1]), NGP_ERR_ARG, "ngp_set_liability_bounds: rows must be strictly increasing and lie in [0, N)");
        REQUIRE(!std::binary_search(ho.begin(), ho.end(), (long long)rows[k]), NGP_ERR_ARG, "ngp_set_liability_bounds: a row is held out (ngp_set_holdout) and bounded");
        REQUIRE(lo[k] < hi[k] && (std::isfinite(lo[k]) || std::isfinite(hi[k])), NGP_ERR_ARG, "ngp_set_liability_bounds: lo < hi, at least one of them finite");
    }
    Liab n;
    n.rows.assign(rows, rows + m); n.lo.assign(lo, lo + m); n.hi.assign(hi, hi + m);
    return commit_liabilities(h, n);
    NGP_CATCH(h)
}

int32_t ngp_get_liability_layout(ngp_handle *h, int64_t *m, int32_t *C) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(h->pm, NGP_ERR_STATE, "panel not set");
    if (m) *m = (int64_t)h->cm.lb.rows.size();
    if (C) *C = h->cm.lb.C;
    return NGP_OK;
    NGP_CATCH(h)
}

/* rows, liab: m entries; thr, sum_thr, sum_thr2: the C - 1 thresholds t_1 .. t_{C-1} (t_1 = 0) and their sums over kept draws (classes
 * only).  Any pointer may be NULL. */
int32_t ngp_get_liability(ngp_handle *h, int64_t *rows, double *liab, double *thr, double *sum_thr, double *sum_thr2, int64_t m, int32_t C) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.on(), NGP_ERR_STATE, "no liability traits on this handle (ngp_set_liability_classes / ngp_set_liability_bounds)");
    REQUIRE(m == (int64_t)lb.rows.size() && C == lb.C, NGP_ERR_ARG, "liability buffers must hold m and C - 1 entries (ngp_get_liability_layout)");
    REQUIRE(h->have_y || !(liab || thr || sum_thr || sum_thr2), NGP_ERR_STATE, "y not set: the liabilities do not exist yet");
    HCHK(hipStreamSynchronize(h->stream));
    if (rows) for (int64_t k = 0; k < m; k++) rows[k] = (int64_t)lb.rows[(size_t)k];
    if (liab) HCHK(hipMemcpy(liab, lb.d_liab, (size_t)m * 8, hipMemcpyDeviceToHost));
    const size_t C1 = (size_t)C + 1, tb = lb.thr_bytes();
    if (thr && tb) HCHK(hipMemcpy(thr, lb.d_thr + 1, tb, hipMemcpyDeviceToHost));
    if (sum_thr && tb) HCHK(hipMemcpy(sum_thr, lb.d_thr + C1 + 1, tb, hipMemcpyDeviceToHost));
    if (sum_thr2 && tb) HCHK(hipMemcpy(sum_thr2, lb.d_thr + 2 * C1 + 1, tb, hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Resume beside ngp_set_state / ngp_set_posterior_sums: what ngp_get_liability gave; a NULL pointer leaves that array as it is. */
int32_t ngp_set_liability_state(ngp_handle *h, const double *liab, const double *thr, const double *sum_thr, const double *sum_thr2, int64_t m, int32_t C) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.on(), NGP_ERR_STATE, "no liability traits on this handle (ngp_set_liability_classes / ngp_set_liability_bounds)");
    REQUIRE(h->have_y, NGP_ERR_STATE, "y not set (ngp_set_y starts the liabilities, this call replaces them)");
    REQUIRE(m == (int64_t)lb.rows.size() && C == lb.C, NGP_ERR_ARG, "liability buffers must hold m and C - 1 entries (ngp_get_liability_layout)");
    if (liab) for (int64_t k = 0; k < m; k++) REQUIRE(std::isfinite(liab[k]), NGP_ERR_ARG, "non-finite liability");
    if (thr && C >= 2) {
        REQUIRE(thr[0] == 0.0, NGP_ERR_ARG, "the first threshold is 0");
        for (int c = 1; c < C - 1; c++) REQUIRE(std::isfinite(thr[c]) && thr[c] >= thr[c - 1], NGP_ERR_ARG, "thresholds must be finite and increasing");
    }
    for (const double *a : {sum_thr, sum_thr2})
        if (a) for (int c = 0; c < C - 1; c++) REQUIRE(std::isfinite(a[c]), NGP_ERR_ARG, "non-finite threshold sum");
    HCHK(hipStreamSynchronize(h->stream));
    if (liab) HCHK(hipMemcpy(lb.d_liab, liab, (size_t)m * 8, hipMemcpyHostToDevice));
    const size_t C1 = (size_t)C + 1, tb = lb.thr_bytes();
    if (thr && tb) HCHK(hipMemcpy(lb.d_thr + 1, thr, tb, hipMemcpyHostToDevice));
    if (sum_thr && tb) HCHK(hipMemcpy(lb.d_thr + C1 + 1, sum_thr, tb, hipMemcpyHostToDevice));
    if (sum_thr2 && tb) HCHK(hipMemcpy(lb.d_thr + 2 * C1 + 1, sum_thr2, tb, hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

/* fallthrough: truncated-normal draws of this handle (chain and probe) whose rejection loop ran out of its 256 rounds; 0 in any sane chain */
int32_t ngp_get_liability_stats(ngp_handle *h, int64_t *fallthrough) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    unsigned long long n = 0;
    if (h->hm.d_tn_fall) {
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipMemcpy(&n, h->hm.d_tn_fall, sizeof n, hipMemcpyDeviceToHost));
    }
    if (fallthrough) *fallthrough = (int64_t)n;
    return NGP_OK;
    NGP_CATCH(h)
}

/* probe of the draw layer (beside ngp_draws_indexed): out[i] = the truncated standard normal on (a[i], b[i]) of stream
 * (seed, chain, iter, kind, index0 + i) */
int32_t ngp_tnormal_indexed(ngp_handle *h, uint64_t iter, uint64_t kind, uint64_t index0, const double *a, const double *b, int64_t n, double *out) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE(a && b && out && n > 0, NGP_ERR_ARG, "bad buffers");
    if ((rc = ensure_tn_fall(h))) return rc;
    DevArray<double> da, db, d;
    if ((rc = da.alloc(h, (size_t)n)) || (rc = db.alloc(h, (size_t)n)) || (rc = d.alloc(h, (size_t)n))) return rc;
    hipError_t e = hipMemcpyAsync(da, a, (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db, b, (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tnormal_indexed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->seed, (uint64_t)h->chain, iter, kind, index0,
                           (const double *)da.get(), (const double *)db.get(), (long long)n, d.get(), h->hm.d_tn_fall.get());
        e = hipMemcpyAsync(out, d, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("tnormal draws: ") + hipGetErrorString(e));
    return NGP_OK;
    NGP_CATCH(h)
}

/* probe of the normal distribution function (ngp_pnorm.h): which 0: out[i] = det_pnorm(a[i]) (b may be NULL); 1: out[i] =
 * det_lpdiff(a[i], b[i]) */
int32_t ngp_debug_pnorm(ngp_handle *h, int32_t which, const double *a, const double *b, int64_t n, double *out) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    REQUIRE((which == 0 || which == 1) && a && (b || which == 0) && out && n > 0, NGP_ERR_ARG, "bad buffers");
    DevArray<double> da, db, d;
    if ((rc = da.alloc(h, (size_t)n)) || (rc = db.alloc(h, (size_t)n)) || (rc = d.alloc(h, (size_t)n))) return rc;
    hipError_t e = hipMemcpyAsync(da, a, (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db, which == 1 ? b : a, (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_pnorm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (int)which, (const double *)da.get(), (const double *)db.get(),
                           (long long)n, d.get());
        e = hipMemcpyAsync(out, d, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, NGP_ERR_HIP, std::string("pnorm probe: ") + hipGetErrorString(e));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Cowles' threshold step ("Cowles' threshold step"; kernels in ngp_threshold.h).  mode 0: Albert-Chib (the
 * default), 1: Cowles' joint Metropolis-Hastings move; sigma > 0 a fixed proposal SD, 0 one that follows the acceptance rate through
 * burn-in.  After ngp_set_liability_classes (which puts the step back to mode 0) and before ngp_set_y. */
int32_t ngp_set_threshold_step(ngp_handle *h, int32_t mode, double sigma) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.on() && lb.C >= 2, NGP_ERR_STATE, "ngp_set_threshold_step: no liability classes on this handle (ngp_set_liability_classes comes first)");
    REQUIRE(!h->have_y, NGP_ERR_STATE, "ngp_set_threshold_step: the phenotypes are set already; the threshold step comes before ngp_set_y");
    REQUIRE(mode == 0 || mode == 1, NGP_ERR_ARG, "ngp_set_threshold_step: mode 0 (Albert-Chib) or 1 (Cowles)");
    REQUIRE(sigma >= 0.0 && std::isfinite(sigma), NGP_ERR_ARG, "ngp_set_threshold_step: sigma > 0 (a fixed proposal SD) or 0 (adapted during burn-in)");
    REQUIRE(mode == 0 || lb.C >= 3, NGP_ERR_ARG, "ngp_set_threshold_step: two classes have no threshold to move (Cowles' step needs C >= 3)");
    if (mode == 0) {
        lb.ts_mode = 0; lb.ts_adapt = false; lb.ts_sigma0 = 0.0;
        lb.d_ts.reset(); lb.d_tg.reset(); lb.d_tpart.reset();
        return NGP_OK;
    }
    const size_t m = lb.rows.size(), nwg = (m + NGP_THR_WG - 1) / NGP_THR_WG;
    DevArray<ThrStep> d_ts;
    DevArray<double> d_tg, d_tpart;
    if ((rc = d_ts.alloc(h, 1)) || (rc = d_tg.alloc(h, (size_t)lb.C + 2)) || (rc = d_tpart.alloc(h, nwg))) return rc;
    const double s0 = sigma > 0.0 ? sigma : 1.0 / std::sqrt((double)m);
    const ThrStep t0{s0, 0, 0};
    HCHK(hipMemcpy(d_ts, &t0, sizeof t0, hipMemcpyHostToDevice));
    lb.ts_mode = 1; lb.ts_adapt = sigma == 0.0; lb.ts_sigma0 = s0;
    lb.d_ts = std::move(d_ts); lb.d_tg = std::move(d_tg); lb.d_tpart = std::move(d_tpart);
    return NGP_OK;
    NGP_CATCH(h)
}

/* mode, the proposal SD in force (0 in mode 0), and the proposals made and taken since ngp_set_y (any pointer may be NULL) */
int32_t ngp_get_threshold_step(ngp_handle *h, int32_t *mode, double *sigma, int64_t *tries, int64_t *accepted) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.on() && lb.C >= 2, NGP_ERR_STATE, "no liability classes on this handle (ngp_set_liability_classes)");
    ThrStep t{0.0, 0, 0};
    if (lb.ts_mode == 1) {
        HCHK(hipStreamSynchronize(h->stream));
        HCHK(hipMemcpy(&t, lb.d_ts, sizeof t, hipMemcpyDeviceToHost));
    }
    if (mode) *mode = lb.ts_mode;
    if (sigma) *sigma = t.sigma;
    if (tries) *tries = (int64_t)t.tries;
    if (accepted) *accepted = (int64_t)t.accepted;
    return NGP_OK;
    NGP_CATCH(h)
}

/* Resume beside ngp_set_liability_state: what ngp_get_threshold_step gave */
int32_t ngp_set_threshold_step_state(ngp_handle *h, double sigma, int64_t tries, int64_t accepted) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.on() && lb.ts_mode == 1, NGP_ERR_STATE, "this handle does not run Cowles' threshold step (ngp_set_threshold_step)");
    REQUIRE(h->have_y, NGP_ERR_STATE, "y not set (ngp_set_y starts the step, this call replaces its state)");
    REQUIRE(sigma > 0.0 && std::isfinite(sigma) && tries >= 0 && accepted >= 0 && accepted <= tries, NGP_ERR_ARG,
            "ngp_set_threshold_step_state: sigma > 0 and 0 <= accepted <= tries");
    const ThrStep t{sigma, (long long)tries, (long long)accepted};
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(lb.d_ts, &t, sizeof t, hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Class probabilities of the held-out records per kept draw ("Class probabilities"; k_holdout_prob).  Needs
 * liability classes and a hold-out mask; before ngp_set_y.  ngp_set_liability_classes switches them off again. */
int32_t ngp_enable_class_probabilities(ngp_handle *h, int32_t on) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.on() && lb.C >= 2 && !h->cm.ho_rows.empty(), NGP_ERR_STATE,
            "ngp_enable_class_probabilities: needs liability classes and held-out records (ngp_set_holdout, then ngp_set_liability_classes)");
    REQUIRE(!h->have_y, NGP_ERR_STATE, "ngp_enable_class_probabilities: the phenotypes are set already; the option comes before ngp_set_y");
    if (!on) { lb.d_sum_prob.reset(); return NGP_OK; }
    if (lb.d_sum_prob) return NGP_OK;
    DevArray<double> d;
    const size_t n = (size_t)lb.C * h->cm.ho_rows.size();
    if ((rc = d.alloc(h, n))) return rc;
    HCHK(hipMemset(d, 0, n * 8));
    lb.d_sum_prob = std::move(d);
    return NGP_OK;
    NGP_CATCH(h)
}

/* sum_prob[C][m]: the sums of the class probabilities over kept draws, class-major, in the row order of the hold-out set; the number
 * of draws is n_fit of ngp_get_holdout */
int32_t ngp_get_class_probabilities(ngp_handle *h, double *sum_prob, int64_t m, int32_t C) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.d_sum_prob, NGP_ERR_STATE, "class probabilities are not enabled on this handle (ngp_enable_class_probabilities)");
    REQUIRE(sum_prob && m == (int64_t)h->cm.ho_rows.size() && C == lb.C, NGP_ERR_ARG, "sum_prob must hold C x m entries (ngp_get_holdout_layout, ngp_get_liability_layout)");
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(sum_prob, lb.d_sum_prob, (size_t)C * (size_t)m * 8, hipMemcpyDeviceToHost));
    return NGP_OK;
    NGP_CATCH(h)
}

/* Resume: what ngp_get_class_probabilities gave */
int32_t ngp_set_class_probabilities(ngp_handle *h, const double *sum_prob, int64_t m, int32_t C) {
    NGP_TRY
    int rc;
    if ((rc = enter(h))) return rc;
    const Liab &lb = h->cm.lb;
    REQUIRE(h->pm && lb.d_sum_prob, NGP_ERR_STATE, "class probabilities are not enabled on this handle (ngp_enable_class_probabilities)");
    REQUIRE(h->have_y, NGP_ERR_STATE, "y not set (ngp_set_y clears the sums, this call replaces them)");
    REQUIRE(sum_prob && m == (int64_t)h->cm.ho_rows.size() && C == lb.C, NGP_ERR_ARG, "sum_prob must hold C x m entries (ngp_get_holdout_layout, ngp_get_liability_layout)");
    for (int64_t k = 0; k < (int64_t)C * m; k++) REQUIRE(std::isfinite(sum_prob[k]) && sum_prob[k] >= 0.0, NGP_ERR_ARG, "a sum of probabilities is finite and not negative");
    HCHK(hipStreamSynchronize(h->stream));
    HCHK(hipMemcpy(lb.d_sum_prob, sum_prob, (size_t)C * (size_t)m * 8, hipMemcpyHostToDevice));
    return NGP_OK;
    NGP_CATCH(h)
}

}  // extern "C"
