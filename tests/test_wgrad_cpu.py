"""Host side of the deferred weight gradients (conan_fgw_amd/wgrad.py) that needs no GPU: the slice rule, the two ctypes job tables, and the
deferral context's bookkeeping."""
import pytest

from conan_fgw_amd import wgrad


def test_slice_rule_of_the_batched_weight_gradients():
    """wgrad._late_slices: ~1 400 workgroups per launch of <= 24 jobs, a multiple of 8 per job, never more than the library's default (one per 128
    rows: the workspace and the reducer are sized by it); the forced knob obeys the same cap."""
    assert wgrad._late_slices(22, 25275) == 64                   # cfg2's backward pass
    assert wgrad._late_slices(40, 15000) == 56                   # more than 24 jobs: the launch is cut at 24
    assert wgrad._late_slices(22, 1280) == 0                     # graph-level layers (default 10 slices): the default stays
    assert wgrad._late_slices(1, 25275) == 0                     # a lone job: 1 400 > its default 198
    keep = wgrad.LATE_SLICES
    try:
        wgrad.LATE_SLICES = 96
        assert wgrad._late_slices(22, 25275) == 96 and wgrad._late_slices(22, 1280) == 0
    finally:
        wgrad.LATE_SLICES = keep
    wgrad.LATE_SLICES_AUTO = False
    try:
        assert wgrad._late_slices(22, 25275) == 0
    finally:
        wgrad.LATE_SLICES_AUTO = True


class _Buf:
    """Stand-in for a contiguous device tensor at a made-up address: all that the job tables read of one."""
    is_cuda = True

    def __init__(self, addr):
        self.addr = addr

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.addr


def _records():
    J = wgrad.Job
    return [J(_Buf(0x1000), 0x2000, 0x3000, None, 300, 50, 128, operands=(_Buf(0x4000), _Buf(0x5000), _Buf(0x6000))),      # slices=0: the library's default
            J(_Buf(0x1100), 0x2100, None, None, 129, 128, 256, slices=8, operands=(_Buf(0x4100), _Buf(0x5000), None)),      # no bias, no device-side row count
            J(_Buf(0x1200), 0x2200, 0x3200, None, 65537, 64, 64, slices=512, weight_ptr=0x7000)]                            # stage 1 done: no operands


def test_slab_job_table():
    jobs = _records()[:2]
    t = wgrad.slab_table(jobs, [j.operands for j in jobs])
    assert len(t) == 2 and isinstance(t[0], wgrad.WgradSlabJob)
    assert [(j.g, j.x, j.m_dev, j.ws, j.M, j.K, j.N, j.slices) for j in t] == \
        [(0x4000, 0x5000, 0x6000, 0x1000, 300, 50, 128, 0), (0x4100, 0x5000, None, 0x1100, 129, 128, 256, 8)]
    assert [j.slices for j in jobs] == [0, 8] and all(j.operands is not None for j in jobs)        # reads only: the records are as before
    assert len(wgrad.slab_table([], [])) == 0


def test_reduce_job_table():
    jobs = _records()
    t = wgrad.reduce_table(jobs)
    assert len(t) == 3 and isinstance(t[0], wgrad.WgradJob)
    assert [(j.ws, j.dW, j.dbias, j.M, j.K, j.N, j.slices) for j in t] == \
        [(0x1000, 0x2000, 0x3000, 300, 50, 128, 0), (0x1100, 0x2100, None, 129, 128, 256, 8), (0x1200, 0x2200, 0x3200, 65537, 64, 64, 512)]
    with pytest.raises(AttributeError):
        jobs[0].slice = 4                                         # a misspelt field fails where it is written, not at the flush


def test_nested_deferrals_close_at_the_outermost():
    assert wgrad.pending() is None
    with wgrad.deferred() as outer:
        assert wgrad.pending() == 0 and isinstance(outer, wgrad.deferred)
        with wgrad.deferred():
            assert wgrad.pending() == 0
        assert wgrad.pending() == 0                                 # the inner context neither flushed nor reset
    assert wgrad.pending() is None
    from conan_fgw_amd import ops
    assert ops.deferred_weight_gradients is wgrad.deferred and ops.flush_weight_gradients is wgrad.flush


def test_a_failing_flush_or_body_leaves_immediate_mode(monkeypatch):
    with pytest.raises(ZeroDivisionError):
        with wgrad.deferred():
            with wgrad.deferred():
                1 / 0
    assert wgrad.pending() is None
    flushes = []

    def boom():
        flushes.append(wgrad.pending())
        raise RuntimeError("flush failed")
    monkeypatch.setattr(wgrad, "flush", boom)
    with pytest.raises(RuntimeError, match="flush failed"):
        with wgrad.deferred():
            with wgrad.deferred():
                pass
            assert flushes == []                                  # the inner exit does not flush
    assert flushes == [0] and wgrad.pending() is None
    with pytest.raises(RuntimeError, match="flush failed"):       # the body raises and the flush raises on top: still immediate afterwards
        with wgrad.deferred():
            raise KeyError("body")
    assert wgrad.pending() is None
