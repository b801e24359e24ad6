// ngp_bayesrc.h -- BayesRCpi marker sets (annotation-informed BayesR; src/functions.jl:291-360, :518-520, :536-544; set-up
// src/mme.jl:384-403, :493-516): what runs BEHIND the sweep.  The lane's rule inside the block chain is eval_rcform (ngp_common.h),
// its coefficient tables are written by k_prep (ngp_kernels.h).
//
// A set has A <= NGP_AMAX annotations and Kc classes, A * Kc <= NGP_RMAX slots, slot i = a * Kc + v.  The chain leaves slot + 1 in
// a locus' delta byte; k_rc_count splits it into the class (delta, from 1) and the annotation (annotCat, from 1) and forms, per
// 256-locus segment in the pattern of k_rssq, sumS of every annotation and the loci of every slot.  k_rc_draw then draws the A
// variances and (estPi) the A Dirichlet rows of pi; k_rc_annot redraws every locus' annotation probabilities.  None of them sits
// in the chain; every one returns at once when the abort word is set.
//
// In a fused pass (ngp_run_many, k_sweep_multi_rc) every chain launches these on its own stream, behind the event of the pass' sweep.
#pragma once
#include "ngp_common.h"

namespace ngp {

struct DRc {  // device arrays of one BayesRCpi set, indexed by the locus inside the set (ncol of them); one entry per marker set
    double *prob;         // annotProb [A][ncol]: 0 where the locus lacks the annotation
    const uint8_t *mask;  // bit a: the locus has annotation a (annotInput, never changed)
    uint8_t *cat;         // annotCat, from 1
    double *sum;          // sum_annot [A][ncol]: kept iterations with annotCat == a + 1
    double *part;         // [nseg][A] segment partials of sumS
    int *cnt;             // [nseg][NGP_RMAX] loci per slot of every segment
    long long nseg;
};

// one wave per 256-locus segment: lane l takes loci l, l+64, l+128, l+192, then the xor butterfly (k_rssq's pattern, per annotation)
__global__ __launch_bounds__(256) void k_rc_count(const DSet *__restrict__ sets, int si, DRc R, const double *__restrict__ beta,
                                                  uint8_t *__restrict__ delta, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long sg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sg >= R.nseg) return;
    const int lane = threadIdx.x & 63;
    const int Kc = sets[si].rcK, A = sets[si].rcA, ns = A * Kc;
    const long long col0 = sets[si].col0, ncol = sets[si].ncol;
    double acc[NGP_AMAX];
    int an[4], sl[4];
    bool bad = false;  // a delta byte that is no slot of the set: the chain did not write it
#pragma unroll
    for (int a = 0; a < NGP_AMAX; a++) acc[a] = 0.0;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const long long l = sg * NGP_SEG + lane + 64 * m;
        an[m] = -1; sl[m] = -1;
        if (l < ncol) {
            int s = (int)delta[col0 + l] - 1;  // slot, as the chain left it
            // out of range (never by this library's chains): kept inside the tables below, and the segment's sums become NaN, so the
            // set's variances and with them the chain are poisoned visibly, as a non-finite variance is everywhere else
            bad = bad || s < 0 || s >= ns;
            s = (s < 0) ? 0 : ((s >= ns) ? ns - 1 : s);
            const int a = s / Kc, v = s - a * Kc;
            an[m] = a; sl[m] = s;
            delta[col0 + l] = (uint8_t)(v + 1);
            R.cat[l] = (uint8_t)(a + 1);
            const double bv = beta[col0 + l];
            const double vc = sets[si].vcls[s];
            if (vc != 0.0) {
                const double b2 = bv * bv;
                const double term = b2 / vc;
#pragma unroll
                for (int b = 0; b < NGP_AMAX; b++)
                    if (b == a) acc[b] = acc[b] + term;
            }
        }
    }
    for (int a = 0; a < A; a++) {
        double x = 0.0;
#pragma unroll
        for (int b = 0; b < NGP_AMAX; b++) x = (b == a) ? acc[b] : x;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
        if (__ballot(bad) != 0ull) x = __builtin_nan("");
        if (lane == 0) R.part[sg * A + a] = x;
    }
    for (int s = 0; s < NGP_RMAX; s++) {
        int n = 0;
#pragma unroll
        for (int m = 0; m < 4; m++) n += __popcll(__ballot(sl[m] == s));
        if (lane == 0) R.cnt[sg * NGP_RMAX + s] = n;
    }
}

// thread a: varBeta[a] = (scale df + sumS[a]) / chi2(df + nNonZero[a]), the region draw's kind with region = a; then (estPi)
// pi[a][.] ~ Dirichlet(nLoci[a][.] + 1) as normalised keyed gammas, index a * Kc + v
__global__ __launch_bounds__(64) void k_rc_draw(DSet *__restrict__ sets, int si, DRc R, double *__restrict__ varBeta, uint64_t seed, uint64_t chain,
                                                uint64_t it, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    DSet *S = &sets[si];
    const int a = threadIdx.x, Kc = S->rcK, A = S->rcA;
    if (a >= A) return;
    double tot = R.part[a];
    for (long long sg = 1; sg < R.nseg; sg++) tot = tot + R.part[sg * A + a];
    long long n[NGP_RMAX], nnz = 0;
    for (int v = 0; v < Kc; v++) {
        long long c = 0;
        for (long long sg = 0; sg < R.nseg; sg++) c += R.cnt[sg * NGP_RMAX + a * Kc + v];
        n[v] = c;
        if (S->vcls[a * Kc + v] != 0.0) nnz += c;
    }
    Rng rr = rng_seed(seed, chain, it, NGP_KIND_REGION_CHI2, ((uint64_t)si << 40) | (uint64_t)a);
    const double ch = rng_chisq(rr, S->df + (double)nnz);
    double tt = S->scale * S->df;
    tt = tt + tot;
    varBeta[a] = tt / ch;
    if (S->estPi) {
        double g[NGP_RMAX], gsum = 0.0;
        for (int v = 0; v < Kc; v++) {
            Rng rg = rng_seed(seed, chain, it, NGP_KIND_R_DIRICHLET, ((uint64_t)si << 40) | (uint64_t)(a * Kc + v));
            g[v] = rng_gamma(rg, (double)n[v] + 1.0);
            gsum = gsum + g[v];
        }
        for (int v = 0; v < Kc; v++) {
            const double p = g[v] / gsum;
            S->pic[a * Kc + v] = p;
            S->logpic[a * Kc + v] = det_log(p);
        }
    }
}

// one thread per locus: annotProb[l, present] ~ Dirichlet(1 + [a == annotCat[l]]) -- gammas of shape 1 or 2 over the present
// annotations in ascending order, divided by their sum; a locus with one annotation keeps exactly 1 (src/functions.jl:322, :541-544)
__global__ __launch_bounds__(256) void k_rc_annot(const DSet *__restrict__ sets, int si, DRc R, uint64_t seed, uint64_t chain, uint64_t it,
                                                  const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x, ncol = sets[si].ncol;
    if (l >= ncol) return;
    const int A = sets[si].rcA;
    const unsigned mk = R.mask[l];
    const int cat = (int)R.cat[l] - 1;
    if (__popc(mk) == 1) {
        for (int a = 0; a < A; a++) R.prob[(size_t)a * ncol + l] = ((mk >> a) & 1u) ? 1.0 : 0.0;
        return;
    }
    double g[NGP_AMAX], gsum = 0.0;
    for (int a = 0; a < A; a++) {
        g[a] = 0.0;
        if ((mk >> a) & 1u) {
            Rng rg = rng_seed(seed, chain, it, NGP_KIND_RC_ANNOT, ((uint64_t)si << 40) | ((uint64_t)l << 3) | (uint64_t)a);
            g[a] = rng_gamma(rg, (a == cat) ? 2.0 : 1.0);
            gsum = gsum + g[a];
        }
    }
    for (int a = 0; a < A; a++) R.prob[(size_t)a * ncol + l] = ((mk >> a) & 1u) ? g[a] / gsum : 0.0;
}

// kept iteration: sum_annot[annotCat[l] - 1][l] += 1
__global__ __launch_bounds__(256) void k_rc_accum(const DSet *__restrict__ sets, int si, DRc R, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x, ncol = sets[si].ncol;
    if (l >= ncol) return;
    const int cat = (int)R.cat[l] - 1;
    if (cat >= 0 && cat < sets[si].rcA) R.sum[(size_t)cat * ncol + l] += 1.0;
}

}  // namespace ngp
