"""bench.py --full: a plain run prints the headline line alone; the result check, the variants, the child runs of the other
configurations and the CPU baselines run only behind the option."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config", "roofline"}
BEHIND_FULL = {"result_check", "hash_table_variant", "two_value_columns_variant", "secondary", "cpu_baseline"}


def test_full_is_an_option_and_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert bench.parse().full is True


def test_child_runs_of_the_other_configurations_ask_for_their_checks(monkeypatch):
    """`secondary` folds each child's property checks in, so the children are run with --full (and without their CPU baseline)."""
    seen = []

    def fake_run(cmd, **kw):
        seen.append(cmd)
        line = {"ms_per_step": 1.0, "value": 1.0, "unit": "rows/s", "steps": 3, "config": {"checks": {"count_ok": True}},
                "roofline": {"frac": 0.1, "whole_call_frac": 0.1, "kernel": "k", "kernels_ms_per_step": {}}}
        return subprocess.CompletedProcess(cmd, 0, stdout=(json.dumps(line) + "\n").encode(), stderr=b"")

    monkeypatch.setattr(subprocess, "run", fake_run)
    out = bench.run_secondary_children()
    assert set(out) == {"c3", "c3_partitioned_probe", "c3sparse", "c3inrange", "c4"}
    assert all("--full" in cmd and "--no-cpu-baseline" in cmd for cmd in seen)
    assert all(v["checks"] == {"count_ok": True} and v["checks_ok"] for v in out.values())


def _run(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--rows", "300001", "--groups", "1000", *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # one JSON line, nothing else on stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone():
    line = _run()
    assert HEADLINE <= set(line) and not BEHIND_FULL & set(line)
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(300001 / (line["ms_per_step"] * 1e-3))


@pytest.mark.gpu
def test_full_run_adds_the_check_and_the_cpu_baseline():
    """(--no-secondary: the variants and the child runs are full-size by construction and have tests of their own)"""
    line = _run("--full", "--no-secondary", "--cpu-sample-rows", "200000")
    assert HEADLINE <= set(line)
    assert line["result_check"]["ok"] is True and line["result_check"]["sum_of_counts"] == 300001
    assert line["cpu_baseline"]["value"] > 0
