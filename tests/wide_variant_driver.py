"""Runs the reduced grid of tests/wide_regimes.py (variant_cases: 769 and 3072 dimensions x {w1_k0, w2_k0} with 2 and 3 tiles per workgroup
over the `random` corpus, which carries the flood, and the rising corpus at 769 dimensions for every RT at k = 32 and k = 112) through the
wide exact scan with the environment's switches (RMU_NT=0: the plain, not non-temporal, w1_k0 / w2_k0, which nothing else reaches;
RMU_NO_SHARED_THR=1: share_thr = 0 -- both read once per process by librmu) and prints what differs from the chain reference.  Executed by
tests/test_wide_regimes_gpu.py in a fresh interpreter per form."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragmeup_amd import FlatIndex  # noqa: E402
from tests import wide_regimes as W  # noqa: E402

nt_env = int(os.environ.get("RMU_NT", "1")) if os.environ.get("RMU_TUNING") == "1" else 1
failures, checked, configs = [], 0, set()
for family, cases in W.families(W.variant_cases()).items():
    f, n = W.run_family(FlatIndex, family, cases, nt_env)
    failures += f
    checked += n
    configs |= {W.plan_wide(c.n, c.nq, c.k, c.dpad, nt_env)["config"] for c in cases}
print("RESULT " + json.dumps({"failures": failures, "checked": checked, "configs": sorted(configs)}))
