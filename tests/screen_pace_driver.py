"""Searches the paced corpus of tests/test_screen_period_gpu.py in a fresh interpreter -- RMU_SCREEN_PACE is read once per process by librmu --
and prints the re-run count and a digest of the answers per k:  python screen_pace_driver.py <rows> <seed> <k> [<k> ...]"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402
from ragmeup_amd import FlatIndex  # noqa: E402

n, seed, ks = int(sys.argv[1]), int(sys.argv[2]), [int(a) for a in sys.argv[3:]]
x = O.make_corpus(n, seed=seed)
q = torch.from_numpy(O.make_queries(x, 1024, seed=seed + 1)[0]).cuda()
idx = FlatIndex(384)
idx.set_ladder(8, 256)
idx.add(x)
out = {}
for k in ks:
    s, r = idx.search(q, k)
    out[str(k)] = {"screened": idx.last_screened(), "digest": hashlib.sha1(r.cpu().numpy().tobytes() + s.cpu().numpy().tobytes()).hexdigest()}
idx.close()
print("RESULT " + json.dumps(out))
