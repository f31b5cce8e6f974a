"""bench.py's plain line and --dump-outputs on the GPU: the line carries the headline and nothing that takes runs of its
own; the dumped arrays are what the timed path computed (checked against the oracle on the sites it samples) and the same
from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import famseq_amd as fs
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    sites = 200000  # ped5: more than the 48 MiB budget holds, so the dump is a sample
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = _bench(["--workload", "ped5", "--sites", str(sites), "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "sites/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        for side in ("cpu_baseline", "elim_engine", "configs_1_ped5", "call_path"):
            assert side not in out
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == ["post", "single", "site_index", "status"]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        assert np.array_equal(a[name], b[name]), name
    idx = a["site_index"].astype(np.int64)
    assert 0 < len(idx) < sites and idx[0] == 0 and np.all(np.diff(idx) > 0) and idx[-1] < sites
    assert a["post"].shape == (len(idx), 5, 3) and a["status"].shape == (len(idx),)

    # the sampled rows against the oracle on the same seeded sites (bench.py's stream, BASELINE configs[1])
    ped = fs.synthetic_pedigree("ped5")
    mo, fa = ped.relations()
    n_head = 256
    lk, flags = fs.synth.gen_batch(mo, fa, n_head, bench_config())
    ref = oracle.OracleModel(ped.ids, ped.mids, ped.fids, ped.genders).bn_batch(lk, flags, threads=4)
    rows = np.nonzero(idx < n_head)[0]
    assert len(rows) > 100
    assert np.array_equal(a["status"][rows], ref[2][idx[rows]].astype(np.float32))
    assert np.array_equal(a["single"][rows], ref[1][idx[rows]])
    np.testing.assert_allclose(a["post"][rows], ref[0][idx[rows]], rtol=1e-9, atol=0)


def bench_config():
    sys.path.insert(0, ROOT)
    import bench

    return bench.WORKLOADS["ped5"][0]
