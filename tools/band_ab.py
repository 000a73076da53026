"""Band seeding of the screening ladder on / off (RMU_OPT_SCREEN_BAND) in ONE process, interleaved: step time per pair, the median
difference and the band-off leg's own pair-to-pair spread, per shape; answers and re-run counts must be identical.  Band off enqueues
exactly what the library enqueued before the option existed, so this is the same-box A/B of the change without a second library.
  python tools/band_ab.py [--shapes 10000000:1024:10,1000000:1024:10,...] [--pairs 6] [--steps 20] [--ladder ratio:first]"""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_shard
from ragmeup_amd import FlatIndex

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="10000000:1024:10,10000000:128:10,10000000:32:10,10000000:16:10,1250000:1024:10,1000000:1024:10,1000000:1024:100")
ap.add_argument("--pairs", type=int, default=6)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--ladder", default="0:0")
a = ap.parse_args()
shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
dev = torch.device("cuda", 0)
nmax = max(s[0] for s in shapes)
x = make_shard(nmax, 384, 1234, dev)
g = torch.Generator(device=dev); g.manual_seed(4321)
bmax = max(s[1] for s in shapes)
qall = x[torch.randperm(nmax, generator=g, device=dev)[:bmax] % min(s[0] for s in shapes)] + 0.1 * torch.randn((bmax, 384), generator=g, dtype=torch.float32, device=dev)
qall /= qall.norm(dim=1, keepdim=True)
ratio, first = (int(v) for v in a.ladder.split(":"))
built = {}
for n, b, k in shapes:
    if n not in built:
        built.clear()                       # one index at a time
        built[n] = FlatIndex(384, capacity_hint=n, device=0)
        built[n].add(x[:n])
        built[n].set_ladder(ratio, first)
    idx = built[n]
    q = qall[:b].contiguous()
    out = (torch.empty((b, k), dtype=torch.float32, device=dev), torch.empty((b, k), dtype=torch.int64, device=dev))

    def leg(on):
        idx.set_screen_band(on)
        for _ in range(3):
            idx.search(q, k, out=out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            idx.search(q, k, out=out)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps, out[0].clone(), out[1].clone(), idx.last_screened(), idx.last_geometry()["launches"]

    on_ms, off_ms, same = [], [], True
    for _ in range(a.pairs):
        f = leg(False); o = leg(True)
        off_ms.append(f[0]); on_ms.append(o[0])
        same = same and torch.equal(f[1], o[1]) and torch.equal(f[2], o[2]) and f[3] == o[3]
    diffs = [f - o for f, o in zip(off_ms, on_ms)]
    print(f"rows {n} batch {b} k {k} ladder {a.ladder} launches {o[4]} screened {o[3]}: off {statistics.median(off_ms):.4f} ms  on {statistics.median(on_ms):.4f} ms  "
          f"median(off - on) {statistics.median(diffs) * 1e3:+.1f} us  pairs faster {sum(d > 0 for d in diffs)}/{a.pairs}  "
          f"spread of off {(max(off_ms) - min(off_ms)) * 1e3:.1f} us  identical={same}", flush=True)
    print("   pairs (off, on) ms: " + "  ".join(f"({f:.4f}, {o:.4f})" for f, o in zip(off_ms, on_ms)), flush=True)
idx.set_screen_band(True)
