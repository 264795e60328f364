"""The two-stage weight gradient of every Linear layer and its deferral (behind the autograd functions of ops.py / visnet_ops.py).

Stage 1 writes per-slice slabs (k_wgrad_lds), stage 2 sums them in a fixed order.  Inside `deferred()` stage 2 of every layer of a backward pass is
postponed and run as ONE launch (conan_wgrad_reduce_batch) by `flush()` instead of 24 launches of ~6 us each; node-level layers postpone stage 1 as
well (one batched launch).  With the library's slice count (LATE_SLICES_AUTO = False) results do not depend on the mode, bit for bit; by default the batch
cuts every job into fewer, longer slices (_late_slices): the same sums in another fixed order (1e-7 relative), 15-18 % less time for the two launches."""
import ctypes

import torch

from ._lib import WgradJob, WgradSlabJob, call, lib, ptr, stream_ptr

f32 = torch.float32
_LATE_STAGE1_ROWS = 65536   # below this row count a weight gradient's slab kernel is postponed to the batched launch
LATE_SLICES = 0             # row slices per postponed job, forced (0 = automatic, below): tools/probe_wgrad_batch.py sweeps it
LATE_SLICES_AUTO = True     # False: the library's default (one slice per 128 rows), i.e. the same slabs — and bits — as the immediate form


def _late_slices(n_jobs: int, M: int) -> int:
    """Row slices per postponed node-level job.  The library's default (one per 128 rows: 198 at cfg2) gives a 22-job batch 4 356 workgroups, each
    writing a 64 KB slab for 8 stages of work; measured in one process (tools/probe_wgrad_batch.py, profiles/r5_wgrad_batch_slices.txt): 198 slices
    249-261 us, 128: 218-227, 96: 212-219, 80: 217, 64: 207-209, 48: 238, 24: 270 — best where a launch (<= 24 jobs) holds ~1 400 workgroups, a
    multiple of 8 per job (the XCD grouping of jobs that share x).  Fixed order of summation either way; not the same order as the default's."""
    dflt = max(1, (M + 127) // 128)
    if LATE_SLICES:
        return LATE_SLICES if LATE_SLICES < dflt else 0           # (never more than the default: the workspace and the reducer are sized by it)
    if not LATE_SLICES_AUTO:
        return 0
    s = 8 * max(1, round(1400 / max(1, min(n_jobs, 24)) / 8))
    return s if s < dflt else 0


class Job:
    """One weight gradient whose sum — and, while `operands` = (g, x, m_dev) is set, whose slab kernel — is still to run; `slices` 0 = the library's
    default.  Deferred mode hands autograd tensors whose values arrive at the flush: only sound if autograd ADOPTS them (it does when it holds the only
    reference and the parameter has no .grad yet; otherwise it copies on the spot), so a job keeps the raw pointers and, in `keep`, the storages —
    never the tensors — and FlatGradients.pack() verifies the adoption."""
    __slots__ = ("ws", "dw_ptr", "db_ptr", "keep", "M", "K", "N", "slices", "weight_ptr", "stream", "operands")

    def __init__(self, ws, dw_ptr, db_ptr, keep, M, K, N, slices=0, weight_ptr=None, stream=None, operands=None):
        self.ws, self.dw_ptr, self.db_ptr, self.keep, self.M, self.K, self.N, self.slices = ws, dw_ptr, db_ptr, keep, M, K, N, slices
        self.weight_ptr, self.stream, self.operands = weight_ptr, stream, operands


_open = None               # None: immediate mode; the list of pending Jobs while deferring
_flushed = {}              # weight data_ptr -> (dW data_ptr, db data_ptr | None) of the last flushes


def pending():
    return None if _open is None else len(_open)      # (None: no deferral is open)


def flushed() -> dict:
    return _flushed        # (the live map: whoever verifies an entry removes it — FlatGradients._flush_deferred)


class deferred:
    """Producers inside this context defer; leaving the outermost one flushes and restores immediate mode, also when the body or the flush raises."""
    def __enter__(self):
        global _open
        self._outermost, _open = _open is None, [] if _open is None else _open
        return self

    def __exit__(self, *exc):
        global _open
        if self._outermost:
            try:
                flush()
            finally:
                _open = None


def claim(weight_ptrs, shape=None, flush_if_pending=True) -> bool:
    """Whether the producer of the gradients of `weight_ptrs` defers: inside a deferral, (K, N) = `shape` batchable where given, none of the weights pending.  A pending
    one is the second use of a weight in this backward (autograd adds the two at once): flush, unless the caller leaves that to a later claim, and run immediately."""
    if _open is None or (shape is not None and not lib().conan_wgrad_batchable(*shape)):
        return False
    twice = any(j.weight_ptr in weight_ptrs for j in _open)
    if twice and flush_if_pending:
        flush()
    return not twice


def job(ws, dw, db, M, K, N, weight_ptr, slices=0, operands=None) -> Job:
    """The record of one producer's workspace and outputs."""
    return Job(ws, dw.data_ptr(), db.data_ptr() if db is not None else None, (dw.untyped_storage(), db.untyped_storage() if db is not None else None),
               M, K, N, slices, weight_ptr, torch.cuda.current_stream(), operands)


def slab_table(jobs, operands) -> ctypes.Array:
    """The job array of conan_linear_wgrad_slabs_batch: stage 1 of `jobs` from their (g, x, m_dev) in `operands`."""
    return (WgradSlabJob * len(jobs))(*[WgradSlabJob(*map(ptr, o), ptr(j.ws), j.M, j.K, j.N, j.slices) for j, o in zip(jobs, operands)])


def reduce_table(jobs) -> ctypes.Array:
    """The job array of conan_wgrad_reduce_batch for `jobs`."""
    return (WgradJob * len(jobs))(*[WgradJob(ptr(j.ws), j.dw_ptr, j.db_ptr, j.M, j.K, j.N, j.slices) for j in jobs])


def flush():
    """Reduce every pending slab set on the current stream (no-op when nothing is pending).  Returns {weight data_ptr: (dW data_ptr,
    db data_ptr | None)} of what was flushed, so that the owner of the parameters can check that autograd adopted those very tensors
    (FlatGradients._flush_deferred does, for dW and db).  The deferred mode is only sound behind that check: use it through
    FlatGradients.backward(), not as a bare `with deferred(): loss.backward()`."""
    if not _open:
        return {}
    cur = torch.cuda.current_stream()
    for st in {j.stream for j in _open} - {cur}:
        cur.wait_stream(st)                                       # slabs written on another stream (the covalent branch runs on one)
    late = [j for j in _open if j.operands is not None]           # node-level layers: stage 1 was postponed as well (see plain)
    if late:
        operands = [j.operands for j in late]
        for j in late:
            j.slices, j.operands = _late_slices(len(late), j.M), None
        call("conan_linear_wgrad_slabs_batch", slab_table(late, operands), len(late), stream_ptr())
        for t in {t for o in operands for t in o if t is not None}:
            t.record_stream(cur)
    call("conan_wgrad_reduce_batch", reduce_table(_open), len(_open), stream_ptr())
    done = {j.weight_ptr: (j.dw_ptr, j.db_ptr) for j in _open}
    for j in _open:
        j.ws.record_stream(cur)
    _open.clear()
    _flushed.update(done)
    return done


def plain(g, x, M, K, N, md, weight, has_bias, rbf=None, gmax=None):
    """dW [N,K] (+ db [N]) = g^T x, or g^T rbf(dist) with rbf = (dist, offset, coeff).  Immediate, or slabs now + batched sum later (see Job)."""
    ws = torch.empty(int(lib().conan_linear_wgrad_ws(M, K, N)), dtype=f32, device=g.device)
    dw, db = torch.empty(N, K, dtype=f32, device=g.device), torch.empty(N, dtype=f32, device=g.device) if has_bias else None
    defer = claim((weight.data_ptr(),), (K, N))
    # Node-level layers (a few ten thousand rows) are latency chains that leave most of the chip idle: in deferred mode their slab
    # kernels are postponed too and all of them run as ONE launch at the flush (conan_linear_wgrad_slabs_batch).  g and x stay alive
    # until then (a node-level pair is 26 MB); edge-level layers already fill the chip and keep their immediate stage 1.
    late = defer and rbf is None and M <= _LATE_STAGE1_ROWS and not (gmax is not None and K > 64)      # (the fp16-plane form has no batched launch)
    if rbf is not None:
        dist, offset, coeff = rbf
        if defer:
            call("conan_rbf_wgrad_slabs", ptr(g), ptr(dist), M, ptr(offset, f32), K, coeff, N, ptr(md), ptr(ws), stream_ptr())
        else:
            call("conan_rbf_wgrad", ptr(g), ptr(dist), M, ptr(offset, f32), K, coeff, N, ptr(md), ptr(dw), ptr(db), ptr(ws), stream_ptr())
    elif gmax is not None and K > 64:
        call("conan_linear_wgrad_scaled", ptr(g), ptr(x), M, K, N, ptr(md), None if defer else ptr(dw), None if defer else ptr(db), ptr(ws),
             ptr(gmax), stream_ptr())
    elif not defer:
        call("conan_linear_wgrad", ptr(g), ptr(x), M, K, N, ptr(md), ptr(dw), ptr(db), ptr(ws), stream_ptr())
    elif not late:
        call("conan_linear_wgrad_slabs", ptr(g), ptr(x), M, K, N, ptr(md), ptr(ws), stream_ptr())
    if defer:
        _open.append(job(ws, dw, db, M, K, N, weight.data_ptr(), operands=(g, x, md) if late else None))
    return dw, db


def shared_x(gs, x, M, K, N, md, weights, has_bias):
    """[plain(g_i, x, ...) for g_i in gs] for several Linear layers of the SAME input and the same width (dk / dv / f_proj of f; q / k / v): the
    slab kernels of the run are ONE launch whose workgroups for one row slice sit next to each other, so x is streamed from HBM once per run
    instead of once per layer (conan_linear_wgrad_slabs_batch; the slabs, and with them the results, are bit for bit those of the separate
    launches).  Falls back to the separate launches where the batched kernel does not apply."""
    n = len(gs)
    usable = n > 1 and bool(lib().conan_wgrad_batchable(K, N)) and K > 64 and N <= 128 and M > _LATE_STAGE1_ROWS      # (node level: the late batch groups such runs itself)
    wptrs = [w.data_ptr() for w in weights]
    if usable and _open is not None:                                    # a weight used twice in one backward: the immediate path of plain handles it
        usable = len(set(wptrs)) == n and claim(wptrs, flush_if_pending=False)
    if not usable:
        return [plain(g, x, M, K, N, md, w, hb) for g, w, hb in zip(gs, weights, has_bias)]
    dev, wsz = x.device, int(lib().conan_linear_wgrad_ws(M, K, N))
    wss = [torch.empty(wsz, dtype=f32, device=dev) for _ in range(n)]
    dws = [torch.empty(N, K, dtype=f32, device=dev) for _ in range(n)]
    dbs = [torch.empty(N, dtype=f32, device=dev) if hb else None for hb in has_bias]
    jobs = [job(wss[q], dws[q], dbs[q], M, K, N, wptrs[q]) for q in range(n)]
    call("conan_linear_wgrad_slabs_batch", slab_table(jobs, [(g, x, md) for g in gs]), n, stream_ptr())
    if _open is not None:
        _open.extend(jobs)
    else:
        call("conan_wgrad_reduce_batch", reduce_table(jobs), n, stream_ptr())
    return list(zip(dws, dbs))


def filter_bwd(g, h1, dist, offset, coeff, w1, w2, M, md, gmax=None):
    """dW1 [F,Gs], db1 [F] of the filter network's first Linear from the gradient g of its output, fused (conan_filter_bwd): the
    input gradient of the second Linear times ssp'(h1) is formed tile by tile in registers and contracted with the regenerated
    rbf(dist) on the spot.  Immediate, or slabs now + batched sum later (see Job)."""
    (F, Gs), dev = w1.shape, g.device
    ws = torch.empty(int(lib().conan_filter_bwd_ws(M, Gs, F)), dtype=f32, device=dev)
    dw, db = torch.empty(F, Gs, dtype=f32, device=dev), torch.empty(F, dtype=f32, device=dev)
    defer = claim((w1.data_ptr(),))
    call("conan_filter_bwd", ptr(g), ptr(h1), ptr(dist), M, ptr(offset, f32), Gs, coeff, ptr(w2), F, ptr(md),
         None if defer else ptr(dw), None if defer else ptr(db), ptr(ws), ptr(gmax), stream_ptr())
    if defer:
        _open.append(job(ws, dw, db, M, Gs, F, w1.data_ptr(), slices=int(lib().conan_filter_bwd_slices(M))))
    return dw, db


def filter_bwd2(g, h1, dist, offset, coeff, w1, w2, M, md, gmax):
    """(dW1 [F,Gs], db1 [F]), (dW2 [F,F], db2 [F]) of the filter network from the gradient g of its output in ONE pass over g and h1
    (conan_filter_bwd2: filter_bwd and the second layer's plain fused).  Immediate, or slabs now + batched sum later (see Job)."""
    (F, Gs), dev = w1.shape, g.device
    ws = torch.empty(int(lib().conan_filter_bwd2_ws(M, Gs, F)), dtype=f32, device=dev)
    slices = int(lib().conan_filter_bwd2_slices(M))
    dw1, db1 = torch.empty(F, Gs, dtype=f32, device=dev), torch.empty(F, dtype=f32, device=dev)
    dw2, db2 = torch.empty(F, F, dtype=f32, device=dev), torch.empty(F, dtype=f32, device=dev)
    p1, p2 = w1.data_ptr(), w2.data_ptr()
    defer = claim((p1, p2))
    call("conan_filter_bwd2", ptr(g), ptr(h1), ptr(dist), M, ptr(offset, f32), Gs, coeff, ptr(w2), F, ptr(md), ptr(gmax),
         None if defer else ptr(dw1), None if defer else ptr(db1), None if defer else ptr(dw2), None if defer else ptr(db2), ptr(ws), stream_ptr())
    if defer:
        cut = slices * (F * Gs + F)
        _open.extend([job(ws[:cut], dw1, db1, M, Gs, F, p1, slices=slices), job(ws[cut:], dw2, db2, M, F, F, p2, slices=slices)])
    return (dw1, db1), (dw2, db2)
