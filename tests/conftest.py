import lzma
import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLDEN = ROOT / "tests" / "golden"
# the reference's shipped model: the stored copy (xz of the identical bytes), or COBALT_REFERENCE_PKL
REFERENCE_PKL = os.environ.get("COBALT_REFERENCE_PKL", "")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (gfx950) GPU and the native HIP library")
    config.addinivalue_line("markers", "slow: long-running test")


def pytest_collection_modifyitems(config, items):
    import torch

    # device_count() does not initialise HIP (is_available() does), so multi-process GPU tests can
    # still spawn their ranks from an uninitialised parent.
    if torch.cuda.device_count() > 0:
        return
    skip = pytest.mark.skip(reason="no GPU in this environment")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session")
def reference_model_bytes():
    """The shipped reference checkpoint (read as bytes only): tests/golden/xgb_model_tree.pkl.xz."""
    if REFERENCE_PKL:
        return Path(REFERENCE_PKL).read_bytes()
    return lzma.decompress((GOLDEN / "xgb_model_tree.pkl.xz").read_bytes())


@pytest.fixture(scope="session")
def reference_booster(reference_model_bytes):
    from cobalt_smart_lender_ai_amd.models.booster import load_pickle_bytes

    return load_pickle_bytes(reference_model_bytes)[1]
