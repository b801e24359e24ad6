"""The coarse seam of the Julia shim on a model of GBLUP terms only (`M` empty: `set_records!` in place of the panel).  No Julia
toolchain exists here, so the route is walked statically, statement by statement, for what breaks on an empty
`sets`: reductions over an empty generator, indexing `sets[1]`, and read-back buffers smaller than what ngp_get_state copies out
of a handle without marker sets (its inert block of 64 columns)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_sampler_body():
    txt = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    a = txt.index("function runSampler!(")
    b = txt.index("\nend # module")
    return txt, [re.sub(r"#[^\n]*", "", ln) for ln in txt[a:b].split("\n")]


def test_empty_marker_sets_route_of_the_coarse_seam():
    txt, body = _run_sampler_body()
    # the route exists: records instead of a panel
    i_if = next(i for i, ln in enumerate(body) if re.search(r"\bif isempty\(sets\)", ln))
    assert "set_records!(h, nData)" in body[i_if + 1]
    i_else = next(i for i in range(i_if, len(body)) if body[i].strip() == "else")
    i_end = next(i for i in range(i_else, len(body)) if body[i].strip() == "end" and "end_panel!" in body[i - 1])
    # sets[1] is only touched where sets is not empty
    for i, ln in enumerate(body):
        if "sets[1]" in ln:
            assert i_else < i < i_end, ln
    # no reduction over a generator of a possibly empty collection without a guard (Julia throws on those)
    for ln in body:
        for m in re.finditer(r"\bsum\(([^()]|\([^()]*\))* for \w+ in (\w+)\)", ln):
            coll = m.group(2)
            guarded = re.search(rf"isempty\({coll}\) \? \d+ : $", ln[:m.start()]) or (i_else < body.index(ln) < i_end)
            assert guarded, ln.strip()
    # the buffers ngp_get_state fills are sized by the handle's P and are never empty
    joined = "\n".join(body)
    call = re.search(r"ccall\(\(:ngp_get_state, LIB\).*?h\.ptr, ycorr, (\w+), (\w+), (\w+), (\w+),", joined, flags=re.S)
    bet, dl, vb, pih = call.groups()
    size = lambda v: re.search(rf"\b{v} = Vector\{{\w+\}}\(undef, ([^)]*\)?)\)", joined).group(1)
    assert size(bet) == "Ptot" and size(dl) == "Ptot"
    assert re.search(r"Ptot = isempty\(sets\) \? RECORDS_ONLY_P : col0", joined)
    assert size(vb).startswith("max(") and size(pih).startswith("2 * max(")
    # ... and that P is the one the header documents and the library allocates
    p = int(re.search(r"const RECORDS_ONLY_P = (\d+)", txt).group(1))
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert re.search(rf"inert block of {p} zero columns", hdr)
    common = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_common.h")).read()
    assert int(re.search(r"#define NGP_BLK (\d+)", common).group(1)) == p
    api = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_api.hip")).read()
    assert "alloc_panel(h, N, NGP_BLK)" in api
    # the caller's arrays are written back on that route too: u / varU of every Z set, b, and ycorr through ngp_get_state
    assert "varU[z] = rs.varU" in joined and "b[1:nfix] .= bfix[1:nfix]" in joined
