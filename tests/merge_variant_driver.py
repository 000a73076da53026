"""Runs the key-merge cases of tests/merge_regimes.py and one search end to end with ONE form of the top-k merge (RMU_MERGE_SELECT, read
once per process by librmu and honoured with RMU_TUNING=1) and prints one RESULT line: the cases that differ from the exact reference,
the pass flags of the searches and a digest of their answers.  Executed by tests/test_merge_regimes_gpu.py in a fresh interpreter per
form: with RMU_MERGE_SELECT=0 every merge goes through merge_wg_kernel -- every wpq, both NPL -- and the form of the merge must not
change a bit of an answer."""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragmeup_amd import FlatIndex, _native  # noqa: E402
from tests import merge_regimes as M  # noqa: E402

select = not (os.environ.get("RMU_TUNING") == "1" and os.environ.get("RMU_MERGE_SELECT") == "0")
fns = M.launchers(_native.lib())
failed, routes = {}, set()
for case in M.CASES:
    route = M.route(case.parts, case.nq, case.k, select=select)
    routes.add(route)
    diff = M.run_key_case(fns, case)
    if diff:
        failed[case.id] = [str(route)] + diff

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev); g.manual_seed(2024)
n = 300_000                                        # several ladder ranges; k = 100 takes the exact threshold ladder from 262 144 rows on
x = torch.randn((n, 384), generator=g, device=dev, dtype=torch.float32)
x /= x.norm(dim=1, keepdim=True)
idx = FlatIndex(384, capacity_hint=n, device=0)
idx.add(x)
idx.set_screen_min_batch(1)
search, sha = {}, hashlib.sha1()
for nq, k, screening in ((96, 10, True), (7, 100, False)):      # the screening ladder (merges to keys, seeded thresholds); the exact scans
    pick = torch.randperm(n, generator=g, device=dev)[:nq]
    q = x[pick] + 0.1 * torch.randn((nq, 384), generator=g, device=dev, dtype=torch.float32)
    q /= q.norm(dim=1, keepdim=True)
    idx.set_screening(screening)
    s, r = idx.search(q, k)
    screened = int(idx.last_screened())
    s, r, pick = s.cpu().numpy(), r.cpu().numpy(), pick.cpu().numpy()
    ok = bool((r[:, 0] == pick).all() and (s[:, 1:] <= s[:, :-1]).all() and (r >= 0).all() and (r < n).all()
              and all(len(set(row.tolist())) == k for row in r) and (screened != 0) == screening)
    search[str(nq)] = {"ok": ok, "screened": screened}
    sha.update(s.tobytes() + r.tobytes())
print("RESULT " + json.dumps({"select": select, "cases": len(M.CASES), "failed": failed, "routes": sorted(map(list, routes)), "search": search,
                              "digest": sha.hexdigest()}))
