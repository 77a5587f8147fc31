"""Distinct queries across ranks, without a GPU: parallel.gather_distinct on a gloo world of two (every rank gets the
broker's merge of every rank's rows), and DistributedAccumulators' refusal of a distinct executor."""
import os
import socket

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from pinot_amd import parse_sql
from pinot_amd.distinct import DistinctResult

SQL = "SELECT DISTINCT a, b FROM t ORDER BY b DESC LIMIT 3"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_result(rank):
    # overlapping rows: (2, "y") on both ranks; a tie class on b = "y" that the cut at 3 falls into
    rows = [[2, "y"], [1, "x"], [9, "y"]] if rank == 0 else [[2, "y"], [5, "z"], [4, "y"]]
    return DistinctResult(["a", "b"], ["INT", "STRING"], rows=rows, present=len(rows))


def _gather_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pinot_amd.parallel import gather_distinct
    out[rank] = gather_distinct(_rank_result(rank), parse_sql(SQL))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_gather_distinct():
    from pinot_amd.reduce import merge_distinct
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_gather_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    expect = merge_distinct([_rank_result(0), _rank_result(1)], parse_sql(SQL))
    # b descending, then a ascending inside the tie class: (5, z), (2, y) once, (4, y); (9, y) is cut
    assert expect == (["a", "b"], [[5, "z"], [2, "y"], [4, "y"]])
    assert out[0] == out[1] == expect


def test_distributed_accumulators_refuse_a_distinct_executor():
    from pinot_amd import _lib as L
    from pinot_amd.parallel import DistributedAccumulators

    class Executor:  # what DistributedAccumulators looks at before it touches the library
        distinct = parse_sql(SQL)
        handle = 1
        hashed = False

    with pytest.raises(L.PinotAmdError, match="gather_distinct"):
        DistributedAccumulators(Executor(), "cpu")
