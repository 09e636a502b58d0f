import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def golden(name):
    """a fixture of tests/golden/; one larger than a committed file may be is stored as <stem>.npz + <stem>.1.npz,
    <stem>.2.npz, ... (tests/golden/make_golden.py:save_parts): the parts are merged, and an array cut over several
    parts is concatenated along its first axis in part order"""
    path = os.path.join(GOLDEN, name)
    parts = sorted(glob.glob(path[:-len(".npz")] + ".[0-9]*.npz"), key=lambda p: int(p.rsplit(".", 2)[1]))
    if not parts:
        return np.load(path)
    merged = dict(np.load(path))
    for p in parts:
        for k, v in np.load(p).items():
            merged[k] = np.concatenate([merged[k], v]) if k in merged else v
    return merged


def rand_rboxes(rng, n, span=1024.0, lo=4.0, hi=100.0):
    """SURVEY.md 8(d) config-1 box distribution."""
    b = np.empty((n, 5), np.float32)
    b[:, 0:2] = rng.uniform(0, span, (n, 2))
    b[:, 2:4] = rng.uniform(lo, hi, (n, 2))
    b[:, 4] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)
    return b


def distinct_scores(rng, n):
    return ((rng.permutation(n).astype(np.float32) + 1) / np.float32(n + 1) * np.float32(0.95)
            + np.float32(0.05))


@pytest.fixture
def rng():
    return np.random.default_rng(1234)
