"""GPU: the engine launches what the shared staging unit (csrc/stage.h) says.  For four small
windows and each of the four search modes, the non-timing fields of engine.launches() equal
what hostcheck_stage reports for the same range and layout policy -- the unit the CPU replays
of first-hit and collect are built on (tests/test_stage_cpu.py) -- and the results equal the
oracle's.
"""
import numpy as np
import pytest

from test_stage_cpu import FORCED, hc, stage  # noqa: F401  (hc is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def one():
    """One context entry, so that a call is one device run over the whole range."""
    import gpuhash
    eng = gpuhash.Engine([0])
    yield eng
    eng.close()


@pytest.mark.parametrize("win", FORCED, ids=[w[0] for w in FORCED])
def test_engine_launches_the_stage(one, hc, oracle, win, request):
    import gpuhash
    name, m, policy, lo, hi, _ = win
    cnt = hi - lo + 1
    assert cnt <= 12000
    hc.hostcheck_set_layout_policy(policy)
    groups, _ = stage(hc, m, lo, hi)
    want = [dict(J=g["J"], C2=g["C2"], EX=g["EX"], digits=g["d"], c=g["c"], nonces=g["nonces"], lo=lo, hi=hi)
            for g in groups]
    h = oracle.hash_range(m, lo, cnt)
    s = np.sort(h)
    request.addfinalizer(lambda: one.set_layout_policy(gpuhash.LAYOUT_AUTO))
    one.set_layout_policy(policy)

    def launched():
        return [{k: r[k] for k in want[0]} for r in one.launches()]

    i = int(np.argmin(h))  # the first of the minima
    assert one.min(m, lo, hi) == (int(h[i]), lo + i) == oracle.min(m, lo, hi)
    assert launched() == want
    assert one.first_below(m, lo, hi, int(s[0])) == (int(h[i]), lo + i)
    assert launched() == want
    target = int(s[cnt // 64])
    idx = np.nonzero(h <= np.uint64(target))[0]
    assert one.collect_below(m, lo, hi, target) == (int(idx.size), [(int(h[k]), lo + int(k)) for k in idx])
    assert launched() == want
    assert (one.hash_range(m, lo, cnt) == h).all()
    assert launched() == want
