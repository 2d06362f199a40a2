"""ps_kf_search / ps_search_by_sim3 draw their scratch from the matcher's arena: the main and contention cases once more in a child
process whose freshly allocated device buffers are filled with 0xFF bytes (tests/test_poisoned_memory_gpu.py does the same for the
earlier calls).  The results must be the ones of the clean run, i.e. the second opinion's."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_main_and_contention_with_poisoned_device_memory():
    env = dict(os.environ, PS_DEBUG_FILL="255")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-k",
                        "members_equal or contention or search_by_sim3_equals or wide_rerun", os.path.join(ROOT, "tests", "test_kfsearch_gpu.py")],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
