"""The plain bench line on one GPU (`bench.py --steps K --warmup W`, no --full): the headline workload alone, its frames checked
against the oracle's digests.  With --dump-outputs a plain run writes what the --full line writes: the arrays of the headline
AND of the `also` workloads, which it then stages, times and checks as well, without their end-to-end legs and CPU baselines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from jsplayer_amd import workloads as wl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *extra],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return json.loads([l for l in res.stdout.decode().splitlines() if l.startswith("{")][-1])


def test_plain_line_is_the_headline_alone():
    doc = _line()
    assert doc["config"]["workload"] == wl.DEFAULT and doc["value"] > 0 and doc["ms_per_step"] > 0
    assert doc["verified"] is True and doc["lookback_fallbacks"] == 0
    assert doc["e2e"] is None and "cpu_baseline" not in doc and "also" not in doc and "dump_outputs" not in doc
    assert doc["roofline"]["reference_fill"] == doc["roofline"]["recorded_fill"]      # no fill measured in the run


def test_plain_line_dumps_every_timed_leg(tmp_path):
    from bench import ALSO_DEFAULT, DUMP_BYTES
    doc = _line("--dump-outputs", str(tmp_path))
    assert doc["verified"] is True and doc["e2e"] is None and "cpu_baseline" not in doc
    legs = [wl.DEFAULT, *ALSO_DEFAULT]
    assert [a["workload"] for a in doc["also"]] == list(ALSO_DEFAULT)
    for a in doc["also"]:
        assert a["verified"] is True and a["value"] > 0 and "e2e" not in a and "cpu_baseline" not in a, a["workload"]
    names = ("frames", "status", "adopted", "significant_changes")
    assert sorted(os.listdir(tmp_path)) == sorted(f"{w}.{k}.npy" for w in legs for k in names)
    assert doc["dump_outputs"]["bytes"] <= DUMP_BYTES
    n = doc["config"]["frames_per_step"]
    status = np.load(tmp_path / f"{wl.DEFAULT}.status.npy")
    assert status.shape == (n,) and not status.any()
