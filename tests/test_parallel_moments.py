"""Form and pivot of the VAR / STDDEV / COVAR accumulators agreed across ranks (parallel.table_layout) on CPU with the
gloo backend, world size 2: the integer form only where every rank's columns stay inside int32, the double form's pivot
from every rank's minimum and maximum, the agreed values in the keyword arguments every rank's executor passes to
pa_query_set_moments (tests/test_gpu_moments.py test_forced_forms_and_pivot shows them reaching the library and deciding
the sections), and the moment sections merging by addition."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pinot_amd import _lib as L
from pinot_amd.parallel import SECTION_DTYPE, SECTION_OP, moments_agreed, reduce_sections, section_runs


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


SQL = ("SELECT k, VAR_POP(m), STDDEV_SAMP(m), VAR_POP(i), STDDEV_POP(d), VAR_SAMP(f), COVAR_POP(i, n), COVAR_SAMP(m, i), "
       "COVAR_POP(i, d) FROM t GROUP BY k")


def _segment(rank):
    from pinot_amd.segment import create_segment
    rng = np.random.default_rng(rank)
    n = 300
    m = rng.integers(0, 1000, size=n).astype(np.int64)
    if rank == 1:
        m[7] = 1 << 40  # only rank 1 holds a LONG value outside int32
    f = (rng.standard_normal(n) * 5).astype(np.float32)
    f[3] = np.nan
    data = {"k": rng.integers(0, 5, size=n).astype(np.int32), "m": m, "n": rng.integers(-9, 9, size=n).astype(np.int64),
            "i": rng.integers(-50, 50, size=n).astype(np.int32), "d": rng.uniform(100.0 * rank, 100.0 * rank + 10, n), "f": f}
    return create_segment("s%d" % rank, data, {"k": "INT", "m": "LONG", "n": "LONG", "i": "INT", "d": "DOUBLE", "f": "FLOAT"},
                          no_dictionary_columns=("m", "d")), data


def _layout_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pinot_amd import parse_sql
    from pinot_amd.parallel import moments_local, table_layout
    q = parse_sql(SQL)
    seg, data = _segment(rank)
    lay = table_layout(q, [seg])
    f = data["f"].astype(np.float64)
    out[rank] = (dict(lay.moments), lay.executor_kwargs()["moments"] == lay.moments, moments_local(q, [seg]),
                 (float(data["m"].min()), float(data["m"].max()), float(data["d"].min()), float(data["d"].max()),
                  float(np.nanmin(f)), float(np.nanmax(f))))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_table_layout_agrees_on_forms_and_pivots():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_layout_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    (lay0, kw0, loc0, mm0), (lay1, kw1, loc1, mm1) = out[0], out[1]
    assert lay0 == lay1 and kw0 and kw1
    INT, DBL = L.PA_MOMENTS_FORM_INTEGER, L.PA_MOMENTS_FORM_DOUBLE
    # rank 0 alone would keep m in the integer form; rank 1's value outside int32 moves both to the double form
    assert loc0["m"][0] is True and loc1["m"][0] is False
    assert lay0[("m", None)][0] == DBL and lay0[("m", "i")] == (DBL, None)
    assert lay0[("i", None)] == (INT, None) and lay0[("i", "n")] == (INT, None) and lay0[("i", "d")] == (DBL, None)
    # the ranks see different minima and maxima: the pivot is the midpoint of the smallest and the largest of all
    for col, (a, b) in (("m", (0, 1)), ("d", (2, 3)), ("f", (4, 5))):
        lo, hi = min(mm0[a], mm1[a]), max(mm0[b], mm1[b])
        assert lay0[(col, None)] == (DBL, lo / 2 + hi / 2), col
        assert (loc0[col][1], loc0[col][2]) == (mm0[a], mm0[b]) and loc0[col][1:] != loc1[col][1:]
    assert set(lay0) == {("d", None), ("f", None), ("i", None), ("i", "d"), ("i", "n"), ("m", None), ("m", "i")}


def test_agreement_rules():
    INT, DBL = L.PA_MOMENTS_FORM_INTEGER, L.PA_MOMENTS_FORM_DOUBLE
    # a rank without a value of the column (all its segments empty) has no say in the pivot
    assert moments_agreed([{"x": [False, 1.0, 3.0]}, {}]) == {("x", None): (DBL, 2.0)}
    assert moments_agreed([{"x": [False, None, None]}, {"x": [False, None, None]}]) == {("x", None): (DBL, 0.0)}
    # a midpoint that is not finite becomes 0; the halves are taken first, so +-DBL_MAX is fine
    big = np.finfo(np.float64).max
    assert moments_agreed([{"x": [False, -big, big]}]) == {("x", None): (DBL, 0.0)}
    assert moments_agreed([{"x": [False, big, big]}]) == {("x", None): (DBL, big)}
    assert moments_agreed([{"x": [False, -np.inf, np.inf]}]) == {("x", None): (DBL, 0.0)}
    assert moments_agreed([{"x": [True, -5.0, 9.0]}, {"x": [True, 0.0, 1.0]}]) == {("x", None): (INT, None)}
    assert moments_agreed([{"x|y": [True, 0.0, 1.0]}, {"x|y": [False, 0.0, 1.0]}]) == {("x", "y"): (DBL, None)}


K = 33


def _partial(rank):
    rng = np.random.default_rng(40 + rank)
    words = rng.integers(-(1 << 40), 1 << 40, K * L.PA_MOMENTS_WORDS).astype(np.int64)
    sums = rng.standard_normal(K * L.PA_MOMENTS_WORDS)
    count = rng.integers(0, 100, K).astype(np.int64)
    return [(L.PA_ACC_COUNT_U64, count), (L.PA_ACC_MOM_I64, words), (L.PA_ACC_MOM_F64, sums)]


def _reduce_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    secs = [(kind, torch.from_numpy(a.copy())) for kind, a in _partial(rank)]
    reduce_sections(secs, all_reduce=True)
    out[rank] = [t.numpy().copy() for _, t in secs]
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_moment_sections_merge_by_addition():
    assert SECTION_OP[L.PA_ACC_MOM_I64] == SECTION_OP[L.PA_ACC_MOM_F64] == dist.ReduceOp.SUM
    assert SECTION_DTYPE[L.PA_ACC_MOM_I64] == torch.int64 and SECTION_DTYPE[L.PA_ACC_MOM_F64] == torch.float64
    # adjacent integer sections (COUNT, integer moments) go out as one collective; the double words as another
    runs = section_runs([(L.PA_ACC_COUNT_U64, 0, K), (L.PA_ACC_MOM_I64, 512, 4 * K), (L.PA_ACC_MOM_F64, 2048, 4 * K)])
    assert [(r[0], r[1]) for r in runs] == [(L.PA_ACC_COUNT_U64, torch.int64), (L.PA_ACC_MOM_F64, torch.float64)]
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_reduce_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    a, b = _partial(0), _partial(1)
    for r in range(world):
        for got, (_, x), (_, y) in zip(out[r], a, b):
            assert np.array_equal(got, x + y)
