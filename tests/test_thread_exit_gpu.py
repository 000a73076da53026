"""GPU: thread exit and process exit of every unit of librmu that owns a thread-local context (csrc/rmu_host.h: the contexts are built
from buffers that free themselves behind each context's own destructor).  tests/thread_exit_driver.py, in a fresh interpreter, makes one
small call into each unit on the main thread, on two worker threads joined one after the other and on the main thread again -- all
results bit-equal -- and exits normally: status 0, `ok` last on stdout, nothing on stderr."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

# what a healthy child may write to stderr: librmu's one notice of an RMU_* variable set without RMU_TUNING=1 (rmu_common.h: rmu_env)
CHATTER = ("librmu: RMU_",)


def test_every_unit_frees_its_context_at_thread_exit_and_at_process_exit():
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "thread_exit_driver.py")], capture_output=True, text=True, timeout=120)
    noise = [ln for ln in out.stderr.splitlines() if ln.strip() and not ln.startswith(CHATTER)]
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines()[-1:] == ["ok"], out.stdout[-2000:]
    assert noise == [], noise
