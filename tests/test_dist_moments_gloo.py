"""The multi-rank merge of the out-of-sample moments on CPU (world_size 2, gloo):
sqlp_amd.dist.merge_moments_in_rank_order all-gathers the ranks' six numbers and merges them in
rank order through twosd_moments_merge (host code, no GPU), so both ranks hold the bits of the
single-process merge.  Per-rank moments are made up; the collective and the merge are the product's."""
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from sqlp_amd import dist as sdist
from sqlp_amd import twosd


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_moments(case, rank):
    if case == "empty_rank" and rank == 0:
        return twosd.Moments(0, 11)                      # every LP of this rank's slice failed
    rng = np.random.default_rng(10 + rank)
    v = 250.0 + (1 + rank) * rng.normal(size=2048 + 5 * rank)
    mean = float(v.mean())
    return twosd.Moments(v.size, rank, mean, float(((v - mean) ** 2).sum()), float(v.min()), float(v.max()))


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out[rank] = {case: sdist.merge_moments_in_rank_order(_rank_moments(case, rank))
                     for case in ("both", "empty_rank")}
    finally:
        dist.destroy_process_group()


def test_two_rank_merge_equals_single_process_merge():
    port = _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
        res = dict(out)
    for case in ("both", "empty_rank"):
        ref = _rank_moments(case, 0).merge(_rank_moments(case, 1))
        assert res[0][case] == ref and res[1][case] == ref          # dataclass equality: every bit
    e = res[0]["empty_rank"]
    r1 = _rank_moments("empty_rank", 1)
    assert (e.n, e.n_bad, e.mean, e.m2, e.min, e.max) == (r1.n, 12, r1.mean, r1.m2, r1.min, r1.max)


def test_single_process_is_identity():
    m = _rank_moments("both", 1)
    assert sdist.merge_moments_in_rank_order(m) is m
