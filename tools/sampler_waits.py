"""Where the sampler's chain wave (wave 0) and its group-sum wave (wave 2) wait on memory, read from the machine code:
python tools/sampler_waits.py [--unit N] [--kernel SUBSTRING] [file.s] > profiles/...

Without a file the translation unit N of the sweep (default 0: k_sweep<false>, the production kernel) is compiled to gfx950 assembly
with the flags of the build (about five minutes).  Two loops of the kernel are found by what only they contain:
  chain wave   the loop with the two tagged-granule stores of dlt (global_store_dwordx2 ... sc1, the second at offset:8)
  wave 2       the lag >= 4 loop of the group sums: the loop over blocks (it holds s_barrier) other than the chain wave's with more than one look (eight sc1 loads, 512 bytes apart)
For each, every s_waitcnt vmcnt is printed with the three instructions before and after it, in the order of the text, with the
loop's memory events (sc1 loads and stores, the other global loads, barriers, the sleeps of its spins) in between as one-line
markers -- enough to see what a wait stands in front of and what is pending when it is reached."""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextgp.jl_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]


def assembly(unit):
    td = tempfile.mkdtemp(prefix="sampler_waits_")
    out = os.path.join(td, f"sweep_{unit}.s")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + [f"-DNGP_INST_DBG={unit}", "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "ngp_sweep_inst.hip")])
    return out


def kernels(lines):
    """{symbol: (first line, last line)} of the functions in the text"""
    starts = [(i, m.group(1)) for i, l in enumerate(lines) if (m := re.match(r"^(_Z\w+):", l))]
    return {name: (i, (starts[k + 1][0] if k + 1 < len(starts) else len(lines))) for k, (i, name) in enumerate(starts)}


def loops_of_blocks(lines, lo, hi):
    """for every line of the kernel the set of loops (named by their header's label) that its basic block belongs to"""
    member = [frozenset()] * (hi - lo)
    cur = frozenset()
    i = lo
    while i < hi:
        l = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):|^; %bb\.\d+:", l)
        if m:
            own = m.group(1)[2:] if m.group(1) else None
            text, k = l, i + 1
            while k < hi and re.match(r"^\s+;", lines[k]) and not lines[k].lstrip().startswith(";;"):
                text += lines[k]; k += 1
            s = set(re.findall(r"Header=(BB\d+_\d+)", text)) | set(re.findall(r"Parent Loop (BB\d+_\d+)", text))
            if own and "Loop Header" in text:
                s.add(own)
            cur = frozenset(s)
        member[i - lo] = cur
        i += 1
    return member


def is_instr(l):
    return l.startswith("\t") and not l.lstrip().startswith((";", "."))


def report(title, lines, lo, member, loop):
    idx = [lo + k for k, s in enumerate(member) if loop in s and is_instr(lines[lo + k])]
    print(f"== {title}: loop {loop}, {len(idx)} instructions")
    ev = re.compile(r"global_(load|store)\w* .*sc1|global_load|global_atomic|s_barrier|s_sleep|s_waitcnt vmcnt")
    shown = set()
    for p, i in enumerate(idx):
        l = lines[i]
        if "s_waitcnt vmcnt" in l:
            print(f"  -- {l.strip()}")
            for q in range(max(0, p - 3), min(len(idx), p + 4)):
                mark = ">>" if q == p else "  "
                print(f"     {mark} {idx[q] - lo + 1:7d}  {lines[idx[q]].strip()}")
                shown.add(q)
        elif ev.search(l) and p not in shown:
            print(f"        {i - lo + 1:7d}  {l.strip()}")
    print()


def main():
    args = sys.argv[1:]
    unit, want = 0, None
    if "--unit" in args:
        k = args.index("--unit"); unit = int(args[k + 1]); del args[k:k + 2]
    if "--kernel" in args:
        k = args.index("--kernel"); want = args[k + 1]; del args[k:k + 2]
    path = args[0] if args else assembly(unit)
    lines = open(path).read().split("\n")
    lines = [l + "\n" for l in lines]
    ks = kernels(lines)
    if want is None:
        want = {0: "k_sweepILb0", 1: "k_sweep_tall", 2: "k_sweep_tup", 3: "k_sweep_r", 5: "k_sweep_dq"}[unit]
    for name, (lo, hi) in ks.items():
        if want not in name:
            continue
        print(f"# {name}  ({os.path.basename(path)}, lines {lo + 1}-{hi})")
        member = loops_of_blocks(lines, lo, hi)
        # chain wave: the granule stores
        chain = None
        for i in range(lo, hi - 3):
            if re.search(r"global_store_dwordx2 .*off sc1", lines[i]) and any(re.search(r"global_store_dwordx2 .*offset:8 sc1", lines[k]) for k in (i + 1, i + 2, i + 3)):
                depth1 = [L for L in member[i - lo]]
                if depth1:
                    chain = sorted(depth1)[0]
                    break
        if chain:
            report("chain wave (sampler wave 0)", lines, lo, member, chain)
        else:
            print("== chain wave: granule stores not found\n")
        # wave 2: looks (the load of the eighth copy, 7 x 512 bytes behind the first) and takes (the zeroing store of that copy), counted per loop
        runs, takes = {}, {}
        for i in range(lo, hi):
            for pat, d in ((r"global_load_dwordx2 .*offset:3584 sc1", runs), (r"global_store_dwordx2 .*offset:3584 sc1", takes)):
                if re.search(pat, lines[i]):
                    for L in member[i - lo]:
                        d[L] = d.get(L, 0) + 1
        blockloops = set()  # loops over the blocks of the sweep: they hold the block's barrier (a spin inside a block does not)
        for i in range(lo, hi):
            if "s_barrier" in lines[i]:
                blockloops |= member[i - lo]
        cands = [L for L, n in runs.items() if n >= 2 and L != chain and L in blockloops]
        outer = [L for L in cands if not any(L != M and _is_child(member, L, M) for M in cands)]
        for L in sorted(outer):
            report(f"group sums, lag >= 4 (sampler wave 2; {runs[L]} looks, {takes.get(L, 0)} takes in the loop)", lines, lo, member, L)
        if not outer:
            print("== wave 2: no loop with more than one look found\n")


def _is_child(member, L, M):
    """L is nested in M: every block of L also belongs to M"""
    return all(M in s for s in member if L in s)


if __name__ == "__main__":
    main()
