"""tools.mqgen.generate_cached: the workload read back from its .npy files is
the generated one, array for array (bench.py's setup relies on it)."""

import dataclasses
import shutil

import numpy as np

from tools import mqgen


def _same(a, b):
    assert a.params == b.params
    for f in dataclasses.fields(mqgen.Workload):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, mqgen.Strings):
            for u, v in ((x.data, y.data), (x.offs, y.offs)):
                assert u.dtype == v.dtype and np.array_equal(u, v), f.name
        elif f.name != "params":
            assert x.dtype == y.dtype and np.array_equal(x, y), f.name


def test_cached_workload_equals_generated():
    kw = dict(n_filters=3001, n_topics=2003, p_shared=0.05)
    d = mqgen._cache_dir(2, kw)
    shutil.rmtree(d, ignore_errors=True)
    try:
        ref = mqgen.generate(2, **kw)
        first = mqgen.generate_cached(2, **kw)  # generates and writes
        assert mqgen.generate_cached(2, load=False, **kw) is None  # the files exist now
        again = mqgen.generate_cached(2, **kw)  # reads back
        _same(ref, first)
        _same(ref, again)
        assert mqgen._cache_dir(2, dict(kw, n_topics=2004)) != d  # other overrides, other files
    finally:
        shutil.rmtree(d, ignore_errors=True)
