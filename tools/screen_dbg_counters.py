"""Per-range debug counters of the screening ladder (debug-kernels build, RMU_SCAN_EXP=7): slow tiles, compactions, appends, cycles in the
slow path / at the pair barrier / in the ring wait / in the pair prologue (clk_pro: barrier release to the first fragment wait), per launch
of ONE search.
  RMU_TUNING=1 RMU_LIB=ragmeup_amd/lib/librmu_dbg.so RMU_SCAN_EXP=7 python tools/screen_dbg_counters.py [rows] [queries] [band: 1 | 0] [spill: 1 | 0] [refresh: 0 | 1]"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_shard
from ragmeup_amd import FlatIndex
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
b = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
dev = torch.device("cuda", 0)
idx = FlatIndex(384, capacity_hint=n, device=0)
x = make_shard(n, 384, 1234, dev); idx.add(x)
if len(sys.argv) > 3:
    idx.set_screen_band(sys.argv[3] != "0")          # RMU_OPT_SCREEN_BAND (default on)
if len(sys.argv) > 4:
    idx.set_screen_spill(sys.argv[4] != "0")         # RMU_OPT_SCREEN_SPILL (default on): spill_tiles instead of slow_tiles in the seeded ranges
if len(sys.argv) > 5:
    idx.set_screen_refresh(sys.argv[5] != "0")       # RMU_OPT_SCREEN_REFRESH (default off): clk_pro, the pair prologue, tells the two apart
q = (x[:b] + 0.1 * torch.randn((b, 384), device=dev)); q /= q.norm(dim=1, keepdim=True)
out = (torch.empty((b, 10), dtype=torch.float32, device=dev), torch.empty((b, 10), dtype=torch.int64, device=dev))
for i in range(2):
    print(f"---- search {i}", file=sys.stderr, flush=True)
    idx.search(q, 10, out=out)
    torch.cuda.synchronize()
