"""Synchronous PS with backup workers on the GPU: 1 PS + 3 workers sharing one card, R = 2, point-to-point over
gloo with host staging (tools/sync_ps_rehearsal.sh).  Covers the HIP model, the fused k-way sum-apply on the PS
and the push / verdict / pull protocol of parallel/sync_ps.py on real hardware; on a node the same example runs
over RCCL with one GPU per process."""
import ast
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_sync_ps_resnet_tiny_one_card():
    N, R, M = 6, 2, 3
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sync_ps_rehearsal.sh"), str(M), "--tiny",
                        "--replicas_to_aggregate", str(R), "--steps", str(N), "--batch", "8", "--image", "32"],
                       capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    m = re.search(r"^\[ps\] (\d+) steps, contributed (\{.*?\}), dropped (\{.*?\}), lost (\[.*?\])$", out, re.M)
    assert m, out[-3000:]
    steps, contributed, dropped, lost = int(m.group(1)), *map(ast.literal_eval, m.group(2, 3, 4))
    assert steps == N and lost == []
    # each of the N steps aggregated exactly R gradients
    assert set(contributed) == set(dropped) == {1, 2, 3}
    assert sum(contributed.values()) == N * R and max(contributed.values()) <= N
    # the workers' own counts agree with the PS's: pushes = contributed + dropped
    rows = re.findall(r"^\[worker (\d+)\] (\d+) pushes, (\d+) contributed, (\d+) dropped", out, re.M)
    assert len(rows) == M, out[-3000:]
    for task, pushes, c, d in rows:
        w = int(task) + 1
        assert (int(c), int(d)) == (contributed[w], dropped[w]) and int(pushes) == int(c) + int(d), (w, out[-3000:])
    losses = [float(x) for x in re.findall(r"global step \d+ loss ([-+.\w]+)", out)]
    assert len(losses) >= N * R and all(math.isfinite(v) for v in losses), losses
