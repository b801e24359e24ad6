// Stand-alone host check of the state table (csrc/ngp_state.h): place() over a chain without and with held-out records, for the three
// layouts.  Meant for a sanitizer build on the host, no device needed:
//   hipcc -x hip --cuda-host-only -std=c++17 -fsanitize=address,undefined -I nextgp.jl_amd/csrc tools/state_layout_check.cpp -o state_layout_check
// Prints the sizes and exits 0 when: the unmasked chain's three images are what they were before hold-out sets existed, the masked
// chain's packed posterior grows by 3 N doubles and its snapshot body by m + 3 N, its sample record not at all, every segment lies
// inside its image without overlap, and copy_segments-style walks over host images stay in bounds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ngp_state.h"

using namespace ngp;

namespace {
struct Model {
    static constexpr int N = 100, P = 192, nvb = 3, nsets = 2, nfix = 2, q = 5, m = 25;
    std::vector<double> ycorr = std::vector<double>(N), beta = std::vector<double>(P), sums = std::vector<double>(3 * P), vb = std::vector<double>(2 * nvb),
                        fix = std::vector<double>(2 * nfix), u = std::vector<double>(2 * q), vu = std::vector<double>(2), yaug = std::vector<double>(m),
                        fit = std::vector<double>(3 * N);
    std::vector<unsigned char> delta = std::vector<unsigned char>(P);
    int64_t iter = 7, rfine = 0;
    uint64_t seed = 1;
    std::vector<uint64_t> fine = std::vector<uint64_t>(nsets);
};

// every pointer is host memory here (the check never touches a device): st.host for all
void describe(Model &M, ChainState &st, bool masked) {
    st.ds.resize(Model::nsets);
    st.nfix = Model::nfix; st.chain64 = 0;
    st.host(SEG_ITER, 0, &M.iter, 8); st.host(SEG_SEED, 0, &M.seed, 8); st.host(SEG_CHAIN, 0, &st.chain64, 8); st.host(SEG_NFIX, 0, &st.nfix, 8);
    st.host(SEG_VARE, 0, &st.sc.varE, 8); st.host(SEG_B, 0, &st.sc.b, 8); st.host(SEG_SUM_VARE, 0, &st.sc.sum_varE, 8); st.host(SEG_SUM_B, 0, &st.sc.sum_b, 8);
    st.host(SEG_NKEPT, 0, &st.sc.nKept, 8); st.host(SEG_NKEPT_F64, 0, &st.nkept_f64, 8);
    st.host(SEG_YCORR, 0, M.ycorr.data(), Model::N * 8); st.host(SEG_BETA, 0, M.beta.data(), Model::P * 8); st.host(SEG_DELTA, 0, M.delta.data(), Model::P);
    st.host(SEG_SUM_BETA, 0, M.sums.data(), Model::P * 8); st.host(SEG_SUM_BETA2, 0, M.sums.data() + Model::P, Model::P * 8);
    st.host(SEG_SUM_DELTA, 0, M.sums.data() + 2 * Model::P, Model::P * 8);
    st.host(SEG_VARBETA, 0, M.vb.data(), Model::nvb * 8); st.host(SEG_SUM_VARBETA, 0, M.vb.data() + Model::nvb, Model::nvb * 8);
    st.host(SEG_FIX, 0, M.fix.data(), Model::nfix * 8); st.host(SEG_SUM_FIX, 0, M.fix.data() + Model::nfix, Model::nfix * 8);
    for (int s = 0; s < Model::nsets; s++) {
        st.host(SEG_FINE, s, &M.fine[(size_t)s], 8);
        st.host(SEG_PI, s, &st.ds[(size_t)s].piHat0, 16); st.host(SEG_SUM_PI, s, &st.ds[(size_t)s].sum_pi0, 16);
    }
    st.host(SEG_U, 0, M.u.data(), Model::q * 8); st.host(SEG_SUM_U, 0, M.u.data() + Model::q, Model::q * 8);
    st.host(SEG_VARU, 0, M.vu.data(), 8); st.host(SEG_SUM_VARU, 0, M.vu.data() + 1, 8); st.host(SEG_VU, 0, M.vu.data(), 16);
    st.host(SEG_RFINE, 0, &M.rfine, 8);
    if (masked) {
        st.host(SEG_YAUG, 0, M.yaug.data(), Model::m * 8);
        st.host(SEG_SUM_FIT, 0, M.fit.data(), Model::N * 8); st.host(SEG_SUM_FIT2, 0, M.fit.data() + Model::N, Model::N * 8);
        st.host(SEG_N_FIT, 0, M.fit.data() + 2 * Model::N, Model::N * 8);
    }
}

int fails = 0;
void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); fails++; }
}

// every segment inside the image, in order, without overlap; a round trip through a host image gives the bytes back
size_t walk(const ChainState &st, const Layout &L, size_t pad, const char *name) {
    const Plan pl = place(st, L, pad);
    size_t end = 0;
    for (auto &a : pl.at) {
        expect(a.off == end, "segments are contiguous and in order");
        end = a.off + a.s->bytes;
    }
    expect(end <= pl.bytes && pl.bytes - end < pad, "the image ends behind its last segment (padded)");
    std::vector<unsigned char> img(pl.bytes + 1, 0xAB);
    for (auto &a : pl.at) std::memcpy(img.data() + a.off, a.s->p, a.s->bytes);   // (what copy_segments does for host segments)
    for (auto &a : pl.at) std::memcpy(a.s->p, img.data() + a.off, a.s->bytes);
    expect(img[pl.bytes] == 0xAB, "nothing is written behind the image");
    std::printf("%-22s %3zu segments %6zu bytes\n", name, pl.at.size(), pl.bytes);
    return pl.bytes;
}
}  // namespace

int main() {
    Model M;
    ChainState plain, masked;
    describe(M, plain, false);
    describe(M, masked, true);
    const size_t N8 = Model::N * 8, P8 = Model::P * 8;
    const size_t post = walk(plain, posterior_layout, 1, "posterior"), smp = walk(plain, sample_layout, 8, "sample record");
    const size_t head = walk(plain, snapshot_head_layout, 1, "snapshot head"), body = walk(plain, snapshot_body_layout, 1, "snapshot body");
    // the unmasked images, counted by hand from the formats at the top of ngp_state.h
    expect(post == 3 * P8 + Model::nvb * 8 + Model::nsets * 16 + Model::nfix * 8 + Model::q * 8 + 8 + 3 * 8, "packed posterior without a mask");
    expect(smp == (8 + 16 + Model::nfix * 8 + Model::q * 8 + 8 + P8 + Model::nvb * 8 + Model::nsets * 16 + Model::P + 7) / 8 * 8, "sample record without a mask");
    expect(head == 32, "snapshot head");
    expect(body == 32 + N8 + P8 + Model::P + Model::nvb * 8 + Model::nsets * 16 + 3 * P8 + Model::nvb * 8 + Model::nsets * 16 + Model::nsets * 8 + 8 +
                       2 * Model::nfix * 8 + 2 * Model::q * 8 + 16 + 8, "snapshot body without a mask");
    const size_t post_m = walk(masked, posterior_layout, 1, "posterior, mask"), smp_m = walk(masked, sample_layout, 8, "sample record, mask");
    const size_t head_m = walk(masked, snapshot_head_layout, 1, "snapshot head, mask"), body_m = walk(masked, snapshot_body_layout, 1, "snapshot body, mask");
    expect(post_m == post + 3 * N8, "packed posterior with a mask: 3 N doubles more");
    expect(smp_m == smp && head_m == head, "sample record and snapshot head do not know the mask");
    expect(body_m == body + Model::m * 8 + 3 * N8, "snapshot body with a mask: m + 3 N doubles more");
    const Plan pm = place(masked, posterior_layout), pb = place(masked, snapshot_body_layout);
    expect(pm.off(SEG_SUM_FIT) == post && pm.off(SEG_N_FIT) == post + 2 * N8, "the hold-out sums end the packed posterior");
    expect(pb.off(SEG_YAUG) == body && pb.off(SEG_N_FIT) == body + Model::m * 8 + 2 * N8, "the hold-out state ends the snapshot body");
    expect(place(plain, posterior_layout).find(SEG_SUM_FIT) == nullptr && place(plain, snapshot_body_layout).find(SEG_YAUG) == nullptr, "no mask: no segment");
    expect(!place(plain, posterior_layout).same_shape(pm) && place(masked, posterior_layout).same_shape(pm), "same_shape tells a masked chain from an unmasked one");
    std::printf(fails ? "%d check(s) failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
