"""tests/fit_dir_ref.py on the CPU: the problem has the zero-degree rows it promises, its totals agree, and the long-double fit
from the sweep's start converges in more than one batch of launches with delta well away from the f that ends it."""
import numpy as np
import pytest

import fit_dir_ref as fd
import fit_ref as fr


@pytest.mark.parametrize("N", [256, 321])
def test_consistent_directed_converges(N):
    pr = fd.consistent_directed(N, 4.0, 450 + N)
    zi, zo = pr["w"] == 0, pr["w2"] == 0
    assert zi.sum() == 2 and zo.sum() == 2 and not np.any(zi & zo)
    assert np.array_equal(pr["T0"], (~zi).astype(float)) and np.array_equal(pr["T0b"], (~zo).astype(float))
    assert pr["w"].sum() == pytest.approx(pr["w2"].sum(), rel=1e-12)  # what a fixed point needs
    ref = fr.fit_directed(fr.numpy_gd(pr, 4.0), pr["T0"], pr["T0b"], pr["w"], pr["w2"], 0.9, delta=1e-3, max_iters=1000)
    K = ref["iters"]
    assert 32 < K < 200
    assert float(ref["f"][K - 1]) < 1e-3 / 1.1 and float(ref["f"][K - 2]) > 1e-3 * 1.1  # the end does not hang on a rounding
    assert ref["eps"][-1] < ref["eps"][0]  # epsilon decayed on the way
