"""Times cudf::filtered_join semi and anti joins on the C3 join shape (bench_configs.make_c3: 500M probe x 50M build rows, 5 % NULLs on
both sides, UNEQUAL) next to inner_join on the same tables, and checks every result count against torch.isin on the valid keys.
usage: python bench_micro/filtered_join_bench.py [scale] [variants dense,sparse,inrange] [reps]
Prints per variant and join: median ms, probe rows/s, and the share of the 8 TB/s peak that the algorithmic bytes take."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C

import torch

from bench_configs import make_c3
from cudf_amd import _lib
from cudf_amd.join import FilteredJoin
from cudf_amd.types import NullEquality

PEAK = 8e12
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
variants = (sys.argv[2] if len(sys.argv) > 2 else "dense,sparse,inrange").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
lib = _lib.load()


def captured(fn, name):
    """A table or tensor make_c3's closures hold (make_c3 returns only its run / check callables)."""
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


for variant in variants:
    run, check, rows, model, (nl, nr, dev) = make_c3(scale, sparse=variant == "sparse", inrange=variant == "inrange")
    L, R = captured(run, "L"), captured(run, "R")
    lk, rk, lvalid, rvalid = (captured(check, x) for x in ("lk", "rk", "lvalid", "rvalid"))
    stream = torch.cuda.current_stream()
    expect_semi = int((torch.isin(lk, rk[rvalid]) & lvalid).sum())
    t0 = time.perf_counter()
    fj = FilteredJoin(R, NullEquality.UNEQUAL, stream=stream)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    out = {}
    for kind in ("semi", "anti"):
        probe = getattr(fj, kind + "_join")
        res = probe(L, stream=stream)
        torch.cuda.synchronize()
        got = res.size()
        want = expect_semi if kind == "semi" else nl - expect_semi
        idx = res.to_torch()
        ordered = bool((idx[1:] > idx[:-1]).all()) if got > 1 else True
        del idx, res
        ms = median_ms(lambda: probe(L, stream=stream))
        # keys (8 B) + validity (1/8 B) per probe row, the match mask written and read (2/8 B), the output (4 B per index); the build
        # state is read once per probe and left out
        bytes_ = nl * (8 + 1 / 8 + 2 / 8) + 4 * got
        out[kind] = ms
        print(f"{variant:8s} {kind}_join  {ms:7.2f} ms  {nl / ms / 1e6:7.2f} Grows/s  {bytes_ / (ms * 1e-3) / PEAK * 100:5.1f} % of peak  "
              f"rows {got} expected {want} count_ok {got == want} ascending {ordered}  [{profile(lambda: probe(L, stream=stream))}]")
    del fj
    res = run()
    c = check(res)
    del res
    ms = median_ms(run)
    print(f"{variant:8s} inner_join {ms:7.2f} ms  {nl / ms / 1e6:7.2f} Grows/s  pairs {c['pairs']} count_ok {c['count_ok']}  "
          f"(filtered_join build {build_ms:.2f} ms; semi / inner {out['semi'] / ms:.2f}, anti / inner {out['anti'] / ms:.2f})")
    del run, check, L, R, lk, rk, lvalid, rvalid
    torch.cuda.empty_cache()
