"""world_size-2 test of veto_amd.distributed.all_gather_eval_state on the gloo backend (CPU tensors, 127.0.0.1): the evaluator
states of uneven shards, one of them without an image, come back as the rank-major list whose concatenation is the unsharded
state."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sgg_eval_split_cases as sc
from veto_amd import distributed as vdist

IMAGE_FIELDS = ("gt_count", "pair_count")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _split():
    """Seven images (one without a GT relation, one without a pair) as a state of CPU tensors."""
    rec = sc.random_split(21, "gloo", [3, 9, 1, 4, 6, 2, 5], 51, {2: "G0", 5: "P0"})
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rec.items()}


def _shard(state, lo, hi):
    off = [0] + torch.cumsum(state["gt_count"], 0).tolist()
    out = {k: state[k][lo:hi].clone() for k in IMAGE_FIELDS}
    out.update({k: state[k][off[lo]:off[hi]].clone() for k in sc.FIELDS})
    return out


# shards per scenario: (rank 0's images, rank 1's images)
SCENARIOS = {"uneven": ((0, 5), (5, 7)), "rank1_empty": ((0, 7), (7, 7)), "rank0_empty": ((0, 0), (0, 7)), "both_empty": ((0, 0), (0, 0))}


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        full = _split()
        got = {name: vdist.all_gather_eval_state(_shard(full, *shards[rank])) for name, shards in SCENARIOS.items()}
        torch.save(got, out % rank)
    finally:
        dist.destroy_process_group()


def test_all_gather_eval_state_world2(tmp_path):
    out = str(tmp_path / "s%d.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    full = _split()
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    for name, shards in SCENARIOS.items():
        for got in (r0[name], r1[name]):      # every rank holds the same list
            assert len(got) == 2
            for rank, st in enumerate(got):      # rank-major, each entry that rank's shard exactly
                want = _shard(full, *shards[rank])
                assert sorted(st) == sorted(want)
                for k in want:
                    assert st[k].dtype == want[k].dtype and torch.equal(st[k], want[k]), (name, rank, k)
            lo, hi = shards[0][0], shards[1][1]
            whole = _shard(full, lo, hi)
            for k in whole:
                assert torch.equal(torch.cat([st[k] for st in got]), whole[k]), (name, k)


def test_single_process_returns_the_state_alone():
    st = _split()
    got = vdist.all_gather_eval_state(st)
    assert len(got) == 1 and got[0] is st
