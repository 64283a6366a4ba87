"""Times cudf::distinct_hash_join's left_join and inner_join on the C3 join shape (bench_configs.make_c3: 500M probe x 50M distinct
build keys, 5 % NULLs on both sides, UNEQUAL) next to cudf::hash_join's left_join and inner_join on the same tables in the same run,
and checks every result against the pair count make_c3 expects.
usage: python bench_micro/distinct_join_bench.py [scale] [variants dense,inrange,sparse] [reps]
Prints per variant and join: median ms of `reps` calls after a warm-up call, probe rows/s, the share of the 8 TB/s peak that the
algorithmic bytes take (distinct_hash_join only), and the per-kernel times of one profiled call."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C

import torch

from bench_configs import make_c3
from cudf_amd import _lib
from cudf_amd.join import JOIN_NO_MATCH, DistinctHashJoin, HashJoin
from cudf_amd.types import NullEquality

PEAK = 8e12
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
variants = (sys.argv[2] if len(sys.argv) > 2 else "dense,inrange,sparse").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
lib = _lib.load()


def captured(fn, name):
    """A table, tensor or number make_c3's closures hold (make_c3 returns only its run / check callables)."""
    return fn.__closure__[fn.__code__.co_freevars.index(name)].cell_contents


def median_ms(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)[len(times) // 2]


def profile(fn):
    lib.cudf_amd_profile_enable(1)
    lib.cudf_amd_profile_reset()
    fn()
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 16)
    lib.cudf_amd_profile_report(buf, len(buf))
    lib.cudf_amd_profile_enable(0)
    return " ".join(f"{ln.split()[0]}={float(ln.split()[2]):.2f}" for ln in buf.value.decode().splitlines())


def built(make):
    t0 = time.perf_counter()
    obj = make()
    torch.cuda.synchronize()
    return obj, (time.perf_counter() - t0) * 1e3


for variant in variants:
    run, check, rows, model, (nl, nr, dev) = make_c3(scale, sparse=variant == "sparse", inrange=variant == "inrange")
    L, R = captured(run, "L"), captured(run, "R")
    lk, rk, expect = captured(check, "lk"), captured(check, "rk"), captured(check, "expect")
    stream = torch.cuda.current_stream()
    dj, dj_build = built(lambda: DistinctHashJoin(R, NullEquality.UNEQUAL, stream=stream))
    hj, hj_build = built(lambda: HashJoin(R, NullEquality.UNEQUAL, stream=stream))
    # results first: the pair count, the keys at the pairs, and left_join's matches = inner_join's right indices in order
    li, ri = dj.inner_join(L, stream=stream)
    lj = dj.left_join(L, stream=stream).to_torch()
    li_t, ri_t = li.to_torch().long(), ri.to_torch()
    hit = lj != JOIN_NO_MATCH
    ok = {"count_ok": li.size() == expect, "keys_equal": bool((lk[li_t] == rk[ri_t.long()]).all()),
          "ascending": bool((li_t[1:] > li_t[:-1]).all()), "left_join_len_ok": lj.numel() == nl,
          "left_join_is_inner": bool((torch.nonzero(hit).flatten() == li_t).all()) and bool((lj[hit] == ri_t).all())}
    pairs = li.size()
    del li, ri, lj, li_t, ri_t, hit
    hl, hr = hj.inner_join(L, stream=stream)
    ok["hash_join_count_ok"] = hl.size() == expect
    del hl, hr
    torch.cuda.empty_cache()
    ms = {}
    for name, obj in (("distinct", dj), ("hash", hj)):
        for kind in ("left", "inner"):
            probe = getattr(obj, kind + "_join")
            fn = lambda: probe(L, stream=stream)  # noqa: E731
            ms[name, kind] = median_ms(fn)
            line = f"{variant:8s} {name:8s} {kind}_join  {ms[name, kind]:8.2f} ms  {nl / ms[name, kind] / 1e6:7.2f} Grows/s"
            if name == "distinct":
                # keys (8 B) + validity (1/8 B) per probe row and the output: 4 B per probe row (left_join); the found rows written
                # and read (8 B per probe row), the mask written and read (2/8 B) and 8 B per pair (inner_join). The random reads of
                # the build table are left out
                bytes_ = nl * (8 + 1 / 8 + 4) if kind == "left" else nl * (8 + 1 / 8 + 8 + 2 / 8) + 8 * pairs
                line += f"  {bytes_ / (ms[name, kind] * 1e-3) / PEAK * 100:5.1f} % of peak"
            print(line + f"  [{profile(fn)}]", flush=True)
    print(f"{variant:8s} pairs {pairs} expected {expect} {ok}  build ms: distinct {dj_build:.2f} hash {hj_build:.2f}  "
          f"distinct / hash: left {ms['distinct', 'left'] / ms['hash', 'left']:.2f} inner {ms['distinct', 'inner'] / ms['hash', 'inner']:.2f}",
          flush=True)
    del dj, hj, run, check, L, R, lk, rk
    torch.cuda.empty_cache()
