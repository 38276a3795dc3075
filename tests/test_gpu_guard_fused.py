"""GPU (-m gpu): guard bands and the placement sweep for the fused decode entry points (tests/checks/guard_fused.py, one section
per test). The check is its own process because a refused launch of the C ABI ends the process: that must fail one test, not the
session. What the run relies on - every draw inside the header's preconditions, the shape lists, the family shares - is proven for
these very arguments by tests/test_guard_bands_host.py."""
import os
import subprocess
import sys

import pytest

from conftest import gpu_ready

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ("gated", "lora", "lora_ids", "shrink", "shrink_ids", "experts", "experts_ffn", "grouped", "rows", "legacy", "python_guards")


@pytest.mark.parametrize("section", SECTIONS)
def test_fused_entry_points_stay_inside_their_outputs_and_need_no_more_than_their_contract(section):
    """Every operand carved at exactly the alignment the header names, inputs between bands of NaN, outputs between bands that reach
    as far as a padded row or column count would: bands untouched, the bytes of the call on fresh tensors, a float64 reference."""
    if not gpu_ready() and not os.path.exists("/dev/kfd") and os.environ.get("BNB_REQUIRE_GPU") != "1":
        pytest.skip("no GPU device on this host")
    assert gpu_ready(), "GPU tests selected but torch.cuda.is_available() is False"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "guard_fused.py"), "--only", section, "--draws", "24", "--seed", "11"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and "GUARD_FUSED OK" in p.stdout, p.stdout[-3000:]
    if section != "python_guards":  # (no draw may be skipped)
        assert f"{section}: 24 draws, seed 11: 24/24 passed" in p.stdout, p.stdout[-3000:]
