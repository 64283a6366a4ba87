"""Helpers for the tests that drive the in-library exchange with peers on one GPU (a loopback world of virtual ranks, one host
thread and one HIP stream per rank): tests/test_loopback_gpu.py and tests/test_distributed_peers_gpu.py."""
import threading

import numpy as np


def run_ranks(world, fn, timeout=300):
    """fn(rank, comm, stream) on one thread per rank of a fresh loopback world; returns the per-rank results."""
    import torch
    from cudf_amd import distributed as D
    comms = D.Communicator.loopback(world)
    out, err = [None] * world, [None] * world

    def body(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(r, comms[r], torch.cuda.Stream())
        except BaseException as e:  # noqa: BLE001 - re-raised on the main thread
            err[r] = e

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    assert not any(t.is_alive() for t in threads), "a rank did not finish (a collective is waiting for a peer)"
    for e in err:
        if e is not None:
            raise e
    return out


def shards(rng, world, rows, groups, empty_rank=None):
    """Ragged shards: rank r holds rows[r] rows of (int64 key, float64 value with ~10% nulls, int32 payload)."""
    out = []
    for r in range(world):
        n = 0 if r == empty_rank else rows[r % len(rows)]
        k = rng.integers(-groups, groups, n, dtype=np.int64)
        v = rng.random(n)
        vv = rng.random(n) > 0.1
        p = rng.integers(0, 1 << 30, n).astype(np.int32)
        out.append((k, v, vv, p))
    return out
