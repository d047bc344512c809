"""`--louvain-level` of `parseargs` (an extension; the reference has no such flag) where no device is needed: the flag is
consulted only when `-c` is absent, and a level that is neither -1 nor >= 1 is refused before anything runs."""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN


def _files(tmp_path):
    src = os.path.join(GOLDEN, "test115")
    for f in ("test.edgelist", "test1col.ecg", "test_n2v.embedding"):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    return [str(tmp_path / f) for f in ("test.edgelist", "test1col.ecg", "test_n2v.embedding")]


def test_with_c_the_flag_is_not_consulted(tmp_path):
    import cge.jl_amd as cg

    g, c, e = _files(tmp_path)
    plain = cg.parseargs(["-g", g, "-c", c, "-e", e, "-l", "20"], exit_on_error=False)
    for level in ("2", "-1", "0", "nonsense"):
        a = cg.parseargs(["-g", g, "-c", c, "-e", e, "-l", "20", "--louvain-level", level], exit_on_error=False)
        assert np.array_equal(a[3], plain[3]) and a[7] == plain[7] == 20
    assert not os.path.exists(g + ".ecg")


def test_without_c_a_bad_level_is_refused_before_louvain_runs(tmp_path):
    import cge.jl_amd as cg
    from cge.jl_amd.args import USAGE, ParseError

    g, _, e = _files(tmp_path)
    for level in ("0", "-2"):
        with pytest.raises(ParseError, match="--louvain-level"):
            cg.parseargs(["-g", g, "-e", e, "--louvain-level", level], exit_on_error=False)
    assert not os.path.exists(g + ".ecg") and "--louvain-level" in USAGE
