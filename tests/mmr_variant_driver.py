"""Runs every case of tests/mmr_regimes.py and one rmu_index_search_mmr call at dim 384 with ONE form of the MMR selection (RMU_MMR_LDS, read
once per process by librmu and honoured with RMU_TUNING=1) and prints one RESULT line: the cases that differ from the exact reference, the
routes the process took, and a digest of every answer.  Executed by tests/test_mmr_regimes_gpu.py in a fresh interpreter with
RMU_TUNING=1 RMU_MMR_LDS=0: every selection goes through k_mmr -- at dim <= 384 too, where the default is k_mmr_lds -- and the form of the
selection must not change a bit of an answer."""
import json
import os
import sys

import torch  # noqa: F401  (first: librmu shares the HIP runtime torch has loaded)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ragmeup_amd  # noqa: E402
from tests import mmr_regimes as M  # noqa: E402

print("RESULT " + json.dumps(M.run_all(ragmeup_amd)))
