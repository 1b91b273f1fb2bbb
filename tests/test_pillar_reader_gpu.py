"""GPU: the fused PointPillars reader (csrc/pillars.hip) and the scatter kernel against the REFERENCE's own module --
tests/golden/pillar_reader.npz, scripts/make_golden_pillars.py -- in training and eval mode, forward + backward, the running
statistics and the canvas.  Tolerances: the project's kernel-golden ones (tests/test_pillar_reader_ref.py)."""
import pytest

from conftest import golden
from test_pillar_reader_ref import check_against_golden

pytestmark = pytest.mark.gpu


def test_fused_reader_against_the_reference_golden(dev):
    check_against_golden(golden("pillar_reader.npz"), dev, expect_fused=True)


def test_composition_on_the_gpu_against_the_reference_golden(dev, monkeypatch):
    """EFG_FUSED_PILLARS=0: the PyTorch composition, the yardstick of scripts/pillar_reader_time.py, on the same golden."""
    monkeypatch.setenv("EFG_FUSED_PILLARS", "0")
    check_against_golden(golden("pillar_reader.npz"), dev, expect_fused=False)
