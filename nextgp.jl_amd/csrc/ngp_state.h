// ngp_state.h -- what a chain holds, as named segments, and its three serialisations as ordered lists of segment ids.  Host only.
//
// A segment is a named run of bytes {id, instance, pointer, bytes}: an array on the device (or a part of one: d_vu holds varU and
// its sum side by side, a half and the whole are different segments over the same array), a word of the handle on the host
// (iteration, seed, fine-seam counters), or a word staged on the host because it lives inside a device struct (DSet, DScal:
// ChainState::ds / sc; the owner of the handle reads them with one copy and writes them back through the setter kernels, whose
// side effects -- logPi, logpic, the cleared counters, iVarE -- belong to the state).  describe() in ngp_api.hip lists the segments
// of a handle; nothing is cached, the model grows with every ngp_add_* call.
//
// A layout is a list of groups of segment ids.  A group is written once per instance (marker set, BayesR set, random-effect set,
// BayesLV set ...), its ids in the order given; a group of one id therefore means "every instance of it, in order".  place() turns
// a layout into offsets and a total size, copy_segments() moves the segments to or from a contiguous image on the device or on
// the host.  Sizes and offsets of the three formats are computed nowhere else.
//
// THE FORMATS (normative; little-endian, doubles unless said otherwise, no padding unless said otherwise)
//
//  A correlated (Tuple) random-effect set of k components (ngp_add_random_set_tuple) has u[q k] (the k components of a level adjacent)
//  and varU[k k] (row-major) wherever a set is written with u[q] and varU below; its q word in the sample file's header and in the
//  snapshot signature carries k - 1 in the bits from 32 up (q < 2^31), and its digest covers the k level vectors and K.
//
//  Packed posterior (ngp_posterior_len, ngp_export_posterior_device, ngp_allreduce_posterior) -- posterior_layout:
//    sum_beta[P] | sum_beta2[P] | sum_delta[P] | sum_varBeta[nvb] | sum_pi[2] per marker set | class sums[K] per BayesR set |
//    fixed-effect sums (every column of every set) | sum_u[q] of every random-effect set, then sum_varU of every set |
//    per BayesLV set sum_c[16], sum_varZeta | per BayesRCpi set sum_annot[A][ncol] | sum_varE | sum_b | nKept (as a double; rounded with
//    llround on the way back).  A BayesRCpi set's pi sums are the class sums of its A K slots, its A variance sums lie in sum_varBeta.
//    A chain with held-out records (ngp_set_holdout, m > 0) appends sum_fit[N] | sum_fit2[N] | n_fit[N] (doubles, zero off the held-out
//    rows); a chain without a mask appends nothing.  A chain with C liability classes (ngp_set_liability_classes) then appends
//    sum_thr[C-1] | sum_thr2[C-1], the sums of the thresholds t_1 .. t_{C-1} (t_1 = 0) and of their squares; any other chain nothing.
//    A chain with class probabilities (ngp_enable_class_probabilities) then appends sum_prob[C][m], class-major over the m held-out
//    records in the order of the hold-out set; any other chain nothing.
//
//  Sample file (ngp_set_sample_file) -- record: sample_layout, padded to a multiple of 8 bytes:
//    header  char[8] magic | int64 P, nvb, nsets, nfix, nclass, record bytes | per marker set int64 {method, K, col0, ncol, variance
//            entries, tuple k}; magic "NGPSMP01": nothing more; "NGPSMP02" (random-effect sets): int64 nrand | int64 q per set;
//            "NGPSMP03" (BayesLV sets): the random-effect part as in 02, also when empty, then int64 nlv | per set int64 marker set, ncov
//            "NGPSMP04" (BayesRCpi sets): the parts of 03, also when empty, then int64 nrc | per set int64 marker set, A, K
//            "NGPSMP05" (C >= 3 liability classes): the parts of 04, also when empty, then int64 nthr = C - 2
//    record  int64 iter (-1: a sweep of the call gave up, the record is not written) | varE | b | b_fixed[nfix] | u[q] of every
//            random-effect set, then varU of every set | beta[P] | varBeta[nvb] | piHat[2] per marker set | class probabilities[K]
//            per BayesR set (the A K slots of a BayesRCpi set, annotation-major) | per BayesLV set c[16] (the first ncov used), varZeta |
//            per BayesRCpi set annotProb[A][ncol] | delta[P] (uint8) | per BayesRCpi set annotCat[ncol] (uint8, from 1) |
//            "NGPSMP05": thr[nthr], the thresholds t_2 .. t_{C-1} of this draw (doubles, directly behind the bytes in front: not aligned)
//
//  Monitored vector of the convergence diagnostics (ngp_enable_diagnostics; ngp_diag.h) -- diag_layout, D doubles:
//    the doubles of a sample record in record order: varE | b | b_fixed[nfix] | u of every random-effect set, then varU of every set |
//    beta[P] | varBeta[nvb] | piHat[2] per marker set | class probabilities | per BayesLV set c[16], varZeta | "NGPSMP05": thr[nthr].
//    Not monitored: iter, delta, annotCat (no doubles) and annotProb[A][ncol] of a BayesRCpi set.
//
//  Snapshot (ngp_save_snapshot / ngp_load_snapshot):
//    char[8] "NGPSNAP2" | int64 N, P, nvb, nsets | snapshot_head_layout: int64 iter, nKept | uint64 seed, chain |
//    model signature (ModelSig in ngp_api.hip): per marker set int64 {method, K + 16 tuple k + 256 (ncov + 32 est_mode) of a
//      BayesLV set, nreg, col0, ncol} | int64 number of fixed-effect sets, bit 62: residual weights, bit 61: random-effect sets,
//      bit 60: held-out records, bit 59: liability traits, bit 58: a fixed residual variance | with weights: uint64 digest of the
//      weights | with held-out records: uint64 digest of their rows | with liabilities: uint64 digest of the augmented rows, C and the
//      classes or bounds | with a fixed residual variance: its value (double) |
//      with random-effect sets: int64 nrand, per set int64 q, uint64 digest of its level
//      coding and K | int64 ncol per fixed-effect set
//    snapshot_body_layout: varE, b, sum_varE, sum_b | ycorr[N] (with residual weights the scaled residual as it lies on the
//      device) | beta[P] | delta[P] (uint8, 0 / 1) | varBeta[nvb] | piHat[2] per set | sum_beta[P] | sum_beta2[P] | sum_delta[P] |
//      sum_varBeta[nvb] | sum_pi[2] per set | uint64 fine_calls per set | int64 nfix | b_fixed[nfix] | sum_b_fixed[nfix] |
//      per BayesR set piHat[K], sum_pi[K] | per random-effect set u[q], sum_u[q], varU, sum_varU, uint64 fine_calls |
//      per BayesLV set the NGP_LV_WORDS doubles of its small state (c, varZeta, their sums, ...), zeta[ncol] |
//      per BayesRCpi set annotProb[A][ncol], sum_annot[A][ncol], annotCat[ncol] (uint8); its signature words are method 6,
//      K = A K slots + a 47-bit digest of the annotation masks from bit 8 up, and nreg = A |
//      with held-out records: yaug[m], sum_fit[N], sum_fit2[N], n_fit[N] (doubles) |
//      with liabilities: liab[m] | with classes also thr[C-1] (t_1 .. t_{C-1}), sum_thr[C-1], sum_thr2[C-1] |
//      with Cowles' threshold step (ngp_set_threshold_step, mode 1): sigma (double), tries, accepted (int64); the mode is folded into
//      the liability digest of the signature, whose bytes in mode 0 are those of a chain that never heard of the step |
//      with class probabilities: sum_prob[C][m]
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "ngp_common.h"

namespace ngp {

enum SegId : int {
    // words of the handle (host)
    SEG_ITER, SEG_SEED, SEG_CHAIN, SEG_NFIX, SEG_FINE, SEG_RFINE,
    // words of DScal and DSet (staged on the host)
    SEG_VARE, SEG_B, SEG_SUM_VARE, SEG_SUM_B, SEG_NKEPT, SEG_NKEPT_F64, SEG_PI, SEG_SUM_PI, SEG_CLS, SEG_SUM_CLS,
    // device arrays: values ...
    SEG_YCORR, SEG_BETA, SEG_DELTA, SEG_VARBETA, SEG_FIX, SEG_U, SEG_VARU, SEG_LV, SEG_ZETA,
    // ... posterior sums ...
    SEG_SUM_BETA, SEG_SUM_BETA2, SEG_SUM_DELTA, SEG_SUM_VARBETA, SEG_SUM_FIX, SEG_SUM_U, SEG_SUM_VARU, SEG_SUM_LV,
    // ... and arrays that hold value and sum side by side, whole
    SEG_VU, SEG_LV_ALL,
    // BayesRCpi sets, per set: annotProb[A][ncol], annotCat[ncol] (uint8, from 1), sum_annot[A][ncol]
    SEG_RC_PROB, SEG_RC_CAT, SEG_SUM_RC,
    // held-out records (described only for a chain that has a mask): yaug[m], and sum_fit[N], sum_fit2[N], n_fit[N] (doubles)
    SEG_YAUG, SEG_SUM_FIT, SEG_SUM_FIT2, SEG_N_FIT
};

struct Seg {
    SegId id;
    int inst;      // which marker set / random-effect set / BayesLV set (0 for what a chain has once)
    void *p;
    size_t bytes;
    bool host;     // p is host memory
};

struct ChainState {
    std::vector<Seg> segs;
    // staging of the words that live inside device structs, and of words whose file form differs from the handle's
    std::vector<DSet> ds;
    DScal sc;
    double nkept_f64 = 0.0;
    int64_t nfix = 0;
    uint64_t chain64 = 0;
    ChainState() = default;
    ChainState(const ChainState &) = delete;  // (the segments point into the staging members)
    ChainState &operator=(const ChainState &) = delete;
    void dev(SegId id, int inst, const void *p, size_t bytes) { segs.push_back({id, inst, const_cast<void *>(p), bytes, false}); }
    void host(SegId id, int inst, void *p, size_t bytes) { segs.push_back({id, inst, p, bytes, true}); }
};

using Layout = std::vector<std::vector<SegId>>;

inline const Layout posterior_layout = {{SEG_SUM_BETA}, {SEG_SUM_BETA2}, {SEG_SUM_DELTA}, {SEG_SUM_VARBETA}, {SEG_SUM_PI}, {SEG_SUM_CLS}, {SEG_SUM_FIX},
                                        {SEG_SUM_U}, {SEG_SUM_VARU}, {SEG_SUM_LV}, {SEG_SUM_RC}, {SEG_SUM_VARE}, {SEG_SUM_B}, {SEG_NKEPT_F64},
                                        {SEG_SUM_FIT}, {SEG_SUM_FIT2}, {SEG_N_FIT}};
inline const Layout sample_layout = {{SEG_ITER}, {SEG_VARE}, {SEG_B}, {SEG_FIX}, {SEG_U}, {SEG_VARU}, {SEG_BETA}, {SEG_VARBETA}, {SEG_PI}, {SEG_CLS},
                                     {SEG_LV}, {SEG_RC_PROB}, {SEG_DELTA}, {SEG_RC_CAT}};
inline const Layout snapshot_head_layout = {{SEG_ITER}, {SEG_NKEPT}, {SEG_SEED}, {SEG_CHAIN}};
inline const Layout snapshot_body_layout = {{SEG_VARE}, {SEG_B}, {SEG_SUM_VARE}, {SEG_SUM_B}, {SEG_YCORR}, {SEG_BETA}, {SEG_DELTA}, {SEG_VARBETA}, {SEG_PI},
                                            {SEG_SUM_BETA}, {SEG_SUM_BETA2}, {SEG_SUM_DELTA}, {SEG_SUM_VARBETA}, {SEG_SUM_PI}, {SEG_FINE}, {SEG_NFIX}, {SEG_FIX},
                                            {SEG_SUM_FIX}, {SEG_CLS, SEG_SUM_CLS}, {SEG_U, SEG_SUM_U, SEG_VU, SEG_RFINE}, {SEG_LV_ALL, SEG_ZETA},
                                            {SEG_RC_PROB, SEG_SUM_RC, SEG_RC_CAT}, {SEG_YAUG, SEG_SUM_FIT, SEG_SUM_FIT2, SEG_N_FIT}};

// Liability traits (ngp_liability.h; described only for a chain that has them): liab[m]; with classes thr[C-1], sum_thr[C-1],
// sum_thr2[C-1].  The ids continue the enumeration, and the groups follow the tables above as tails: place() appends a table's tail, so
// the tables themselves stay what every chain without liabilities is written by.  SEG_THR_SMP: the drawn thresholds t_2 .. t_{C-1}
// (described for C >= 3 only), the sample record's tail behind its bytes.
constexpr SegId SEG_LIAB = (SegId)(SEG_N_FIT + 1), SEG_THR = (SegId)(SEG_N_FIT + 2), SEG_SUM_THR = (SegId)(SEG_N_FIT + 3), SEG_SUM_THR2 = (SegId)(SEG_N_FIT + 4),
                SEG_THR_SMP = (SegId)(SEG_N_FIT + 5);
inline const Layout liability_posterior_tail = {{SEG_SUM_THR}, {SEG_SUM_THR2}};
inline const Layout liability_snapshot_tail = {{SEG_LIAB, SEG_THR, SEG_SUM_THR, SEG_SUM_THR2}};
inline const Layout liability_sample_tail = {{SEG_THR_SMP}};
inline const Layout *tail_of(const Layout &L) {
    return &L == &posterior_layout ? &liability_posterior_tail : &L == &snapshot_body_layout ? &liability_snapshot_tail
         : &L == &sample_layout ? &liability_sample_tail : nullptr;
}

// The monitored vector of the convergence diagnostics (ngp_diag.h): the doubles of a sample record in record order, without iter (not a
// double) and the BayesRCpi annotProb block (A P words); the drawn thresholds end it as they end the record (a group without instances
// places nothing, so the table needs no tail)
inline const Layout diag_layout = {{SEG_VARE}, {SEG_B}, {SEG_FIX}, {SEG_U}, {SEG_VARU}, {SEG_BETA}, {SEG_VARBETA}, {SEG_PI}, {SEG_CLS}, {SEG_LV}, {SEG_THR_SMP}};

// Ordered traits on the scale of the trait (ngp_threshold.h), a second tail behind the liabilities', built the same way.  Cowles'
// threshold step (ngp_set_threshold_step, mode 1; described for such a chain only): SEG_THR_STEP = sigma (double) | tries | accepted
// (int64), in the snapshot.  Class probabilities of the held-out records (ngp_enable_class_probabilities; described only where they
// are on): SEG_SUM_PROB = sum_prob[C][m], class-major, m the held-out records in the order of the hold-out set -- the end of the
// packed posterior and of the snapshot body.  The sample record has no such tail.
constexpr SegId SEG_THR_STEP = (SegId)(SEG_N_FIT + 6), SEG_SUM_PROB = (SegId)(SEG_N_FIT + 7);
inline const Layout ordered_posterior_tail = {{SEG_SUM_PROB}};
inline const Layout ordered_snapshot_tail = {{SEG_THR_STEP}, {SEG_SUM_PROB}};
inline const Layout *ordered_tail_of(const Layout &L) {
    return &L == &posterior_layout ? &ordered_posterior_tail : &L == &snapshot_body_layout ? &ordered_snapshot_tail : nullptr;
}

// a layout applied to a chain: every segment with its byte offset, and the size of the whole
struct Plan {
    struct At { const Seg *s; size_t off; };
    std::vector<At> at;
    size_t bytes = 0;
    const At *find(SegId id, int inst = 0) const {
        for (auto &a : at) if (a.s->id == id && a.s->inst == inst) return &a;
        return nullptr;
    }
    size_t off(SegId id) const { return find(id)->off; }           // (of a segment every chain has)
    size_t size(SegId id) const { return find(id)->s->bytes; }
    // the same segments of the same lengths in the same order: two chains of one model
    bool same_shape(const Plan &o) const {
        if (at.size() != o.at.size()) return false;
        for (size_t i = 0; i < at.size(); i++)
            if (at[i].s->id != o.at[i].s->id || at[i].s->bytes != o.at[i].s->bytes) return false;
        return true;
    }
};

// pad: the total is rounded up to a multiple of it
inline Plan place(const ChainState &st, const Layout &L, size_t pad = 1) {
    Plan pl;
    const Layout *tail = tail_of(L);
    for (const Layout *part : {&L, tail, ordered_tail_of(L)}) {
        if (!part) continue;
        for (auto &group : *part)
            for (auto &first : st.segs) {  // the instances of a group: those of its first id, in the order describe() lists them
                if (first.id != group[0]) continue;
                for (SegId id : group)
                    for (auto &s : st.segs)
                        if (s.id == id && s.inst == first.inst) { pl.at.push_back({&s, pl.bytes}); pl.bytes += s.bytes; }
            }
    }
    pl.bytes = (pl.bytes + pad - 1) / pad * pad;
    return pl;
}

// gather (to_image) or scatter the segments of a plan to / from a contiguous image in device or host memory; returns once the
// copies are through
inline hipError_t copy_segments(const Plan &pl, void *image, bool image_host, bool to_image, hipStream_t stream) {
    hipError_t e = hipSuccess;
    for (auto &a : pl.at) {
        if (a.s->bytes == 0) continue;
        void *im = (unsigned char *)image + a.off;
        void *dst = to_image ? im : a.s->p;
        const void *src = to_image ? a.s->p : im;
        const bool dst_host = to_image ? image_host : a.s->host, src_host = to_image ? a.s->host : image_host;
        if (dst_host && src_host) { std::memcpy(dst, src, a.s->bytes); continue; }
        const hipMemcpyKind kind = src_host ? hipMemcpyHostToDevice : (dst_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
        if ((e = hipMemcpyAsync(dst, src, a.s->bytes, kind, stream)) != hipSuccess) break;
    }
    const hipError_t es = hipStreamSynchronize(stream);
    return e != hipSuccess ? e : es;
}

}  // namespace ngp
