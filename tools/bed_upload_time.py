"""Times a genotype panel from host memory (or a file) to a finished panel on the device, three ways:
  (a) bed   ngp_panel_columns_bed from an in-memory packed array (2 bits per genotype cross PCIe, decoded on the device)
  (b) u8    ngp_panel_columns_u8 from the decoded codes (1 byte per genotype)
  (c) ngp   ngp_load_panel_file on a bits=2 panel file with the same codes (unpacked on the host)
for fp32 and byte tiles, (a) and (b) also with a row map (a permutation of the file's samples; (b) is given the gathered codes, the
host gather is not timed).  Wall time of the column upload and of ngp_end_panel (mpm and the Gram window) apart, every leg REPS times
on a fresh handle, all three times printed.  The inputs hold no missing call, so that (b) and (c) can run.
python tools/bed_upload_time.py N P [reps] [--no-file]"""
import os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg
ngp = load_pkg()
args = [a for a in sys.argv[1:] if not a.startswith("--")]
N, P = int(args[0]), int(args[1])
REPS = int(args[2]) if len(args) > 2 else 3
rng = np.random.default_rng(1)
BW = min(P, 2048)                            # a random block of columns, repeated: the upload does not care
blk = rng.integers(0, 3, size=(N, BW), dtype=np.uint8)
G8 = np.empty((N, P), dtype=np.uint8, order="F")
for a in range(0, P, BW):
    G8[:, a:a + BW] = blk[:, :min(BW, P - a)]
nb = (N + 3) // 4
code = np.zeros((4 * nb, BW), dtype=np.uint8)
code[:N] = np.array([3, 2, 0], dtype=np.uint8)[blk]
pk = np.ascontiguousarray((code[0::4] | (code[1::4] << 2) | (code[2::4] << 4) | (code[3::4] << 6)).T)
packed = np.empty((P, nb), dtype=np.uint8)
for a in range(0, P, BW):
    packed[a:a + BW] = pk[:min(BW, P - a)]
rows = rng.permutation(N).astype(np.int64)
G8m = np.empty((N, P), dtype=np.uint8, order="F")
gm = np.asfortranarray(blk[rows])
for a in range(0, P, BW):
    G8m[:, a:a + BW] = gm[:, :min(BW, P - a)]
del code, pk, gm
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "panel2.ngp")
if "--no-file" not in sys.argv:
    ngp.write_panel_file(path, G8, bits=2)


def leg(storage, what, mapped):
    s = ngp.Sampler(device=0, seed=1, chain=0, storage=storage)
    t = time.perf_counter()
    if what == "ngp":
        s.load_panel_file(path, centre=True)          # (begin, columns and end in one call)
        return time.perf_counter() - t, float("nan")
    s.begin_panel(N, P)
    if what == "bed":
        s.panel_columns_bed(0, packed, N, rows=rows if mapped else None, missing="error", centre=True)
    else:
        s.panel_columns(0, G8m if mapped else G8, centre=True)
    t1 = time.perf_counter() - t
    t = time.perf_counter(); s.end_panel(); t2 = time.perf_counter() - t
    return t1, t2


print(f"N={N} P={P}: packed {packed.nbytes / 1e9:.2f} GB, codes {G8.nbytes / 1e9:.2f} GB, {REPS} runs per leg", flush=True)
if "--dry" in sys.argv:                      # inputs only (no device)
    sys.exit(0)
w = ngp.Sampler(device=0, seed=1, chain=0)   # warm-up: the kernels' code objects are loaded before anything is timed
w.begin_panel(N, 64); w.panel_columns_bed(0, packed[:64], N, rows=rows, missing="error"); w.panel_columns(0, G8[:, :64], centre=True); w.end_panel()
del w
for storage in (None, "u8"):
    for mapped in (False, True):
        legs = [x for x in ("bed", "u8", "ngp") if not (x == "ngp" and (mapped or "--no-file" in sys.argv))]
        runs = {x: [] for x in legs}
        for _ in range(REPS):                # the legs alternate: a busy host hits them alike
            for what in legs:
                runs[what].append(leg(storage, what, mapped))
        for what in legs:
            ts = runs[what]
            tot = sorted(a + (0.0 if b != b else b) for a, b in ts)
            print(f"storage={storage or 'f32'} rows={'map' if mapped else 'file'} {what:>3}: total min {tot[0]:.3f} median {tot[len(tot) // 2]:.3f} max {tot[-1]:.3f} s | "
                  f"columns {' '.join(f'{a:.3f}' for a, _ in ts)} | end_panel {' '.join(f'{b:.3f}' for _, b in ts)}", flush=True)
if os.path.exists(path):
    os.remove(path)
os.rmdir(tmp)
