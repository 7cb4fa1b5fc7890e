"""The bench line stays parseable: < 8 KB, strict JSON, the contract's fields present (the 25 KB line of
round 5 came back `parsed: null` from the driver).  Inputs: the fat lines round 5 committed under profiles/ and a synthetic
worst case; benchdata/line.py is pure Python."""
import glob
import json
import os

import pytest

from benchdata import line as benchline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline")


def _strict(text):
    def bad(tok):
        raise ValueError("non-standard JSON constant %r" % tok)
    return json.loads(text, parse_constant=bad)


def _fat_lines():
    out = []
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r05", "r05[u-y]_bench*.json"))):
        txt = open(f).read().strip().splitlines()[-1]
        if len(txt) > 8192:
            out.append((os.path.basename(f), json.loads(txt)))
    return out


FAT = _fat_lines()


def test_round5_lines_exist_and_were_too_big():
    assert len(FAT) >= 3 and all(len(json.dumps(r)) > 20000 for _, r in FAT)


@pytest.mark.parametrize("name,res", FAT, ids=[n for n, _ in FAT])
def test_fat_lines_compact_below_the_limit(name, res):
    line = benchline.dumps(res, "bench_detail.json")
    assert len(line.encode()) < 8192 and "\n" not in line
    back = _strict(line)
    for k in CONTRACT:
        assert k in back, k
    assert back["value"] == pytest.approx(res["value"], rel=1e-4) and back["ms_per_step"] == pytest.approx(res["ms_per_step"], rel=1e-4)
    assert back["config"]["workload"] and "model" not in back["config"]
    roof = back["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-3)
    assert roof["unit"] in ("GB/s", "TFLOP/s") and "traffic" in roof
    if "other_configs" in res:
        for k, v in res["other_configs"].items():
            got = back["other_configs"][k]
            for f in ("ms_per_step", "audio_s_per_s", "latency_ms"):
                if f in v:
                    assert got[f] == v[f]
    assert back["detail"] == "bench_detail.json"


def test_worst_case_still_fits_and_is_strict_json():
    name, res = FAT[0]
    res = json.loads(json.dumps(res))
    res["roofline"]["classes"] = res["roofline"]["classes"] * 40
    res["roofline"]["frac"] = float("nan")  # a NaN must not reach the line as a bare token
    res["config"]["workload"] = "w" * 5000
    res["cpu_baseline"] = {"value": 23.6, "unit": "audio-s/s", "cores": 16, "kind": "reference", "sample": "s" * 3000,
                           "threads_tried": {str(i): 1.0 for i in range(200)}, "host_cores": 256}
    res["other_configs"] = {("leg%d" % i): dict(res["other_configs"]["libritts_hifigan"]) for i in range(40)}
    line = benchline.dumps(res, "bench_detail.json")
    assert len(line.encode()) < 8192
    back = _strict(line)
    assert back["roofline"]["frac"] is None and back["cpu_baseline"]["kind"] == "reference"
    for k in CONTRACT:
        assert k in back


def test_bench_py_prints_through_the_compactor():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "print(json.dumps(res)" not in src and "benchline.dumps(res" in src


def test_plain_line_without_roofline():
    """A plain `bench.py` run (no --full) has no per-launch conv events and so no `roofline`: the line leaves it out and keeps
    the headline fields as they are."""
    name, res = FAT[0]
    res = json.loads(json.dumps(res))
    for k in ("roofline", "box", "other_configs", "cpu_baseline"):
        res.pop(k, None)
    back = _strict(benchline.dumps(res))
    assert "roofline" not in back and "detail" not in back
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert back[k] == (pytest.approx(res[k], rel=1e-4) if isinstance(res[k], float) else res[k]), k


def test_dump_outputs_writes_float32_arrays(tmp_path):
    """--dump-outputs: the waveform batch as one array, long-form's per-sentence waveforms as one array each, float32."""
    import numpy as np
    import torch

    import bench
    w = torch.randn(2, 1, 600, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "batch"), w)
    got = np.load(tmp_path / "batch" / "waveform.npy")
    assert got.dtype == np.float32 and got.shape == (2, 1, 600) and np.array_equal(got, w.numpy())
    waves = [torch.randn(n) for n in (500, 700)]
    bench.dump_outputs(str(tmp_path / "long"), waves)
    for i, x in enumerate(waves):
        got = np.load(tmp_path / "long" / ("waveform_%02d.npy" % i))
        assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    assert sorted(os.listdir(tmp_path / "long")) == ["waveform_00.npy", "waveform_01.npy"]


def test_bench_cli_full_dump_outputs_and_steps():
    import subprocess
    import sys
    run = lambda *args: subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True,
                                       text=True, timeout=120)
    h = run("--help")
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    bad = run("--steps", "0")
    assert bad.returncode == 2 and "--steps" in bad.stderr
