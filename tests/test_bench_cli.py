"""bench.py's launch contract on the CPU (no GPU work): --gpus N must equal the number
of ranks torch.distributed.run started (WORLD_SIZE), so a bare `--gpus 8` fails loudly
instead of printing a one-rank line."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_must_match_world_size():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr and "--nproc-per-node 8" in r.stderr


def test_load_traffic_matches_config_exactly(tmp_path):
    sys.path.insert(0, ROOT)
    import json
    import bench
    cfg = {"k": 10, "m": 4, "shard_bytes": 1 << 20, "stripes": 256, "erase": [0, 1, 2, 3]}
    p = tmp_path / "t.json"
    p.write_text(json.dumps({"config": cfg, "encode_bytes_per_launch": 5, "decode_bytes_per_launch": 6}))
    assert bench.load_traffic(str(p), cfg)[:2] == (5, 6)
    assert bench.load_traffic(str(p), {**cfg, "stripes": 128}) == (None, None, None)
    assert bench.load_traffic(str(tmp_path / "missing.json"), cfg) == (None, None, None)


def test_committed_traffic_matches_the_default_bench_config():
    """profiles/hbm_traffic.json (the rocprofv3 PMC bytes the line quotes as `traffic`)
    is keyed by the default bench config, layout included."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args([])
    cfg = {"k": a.k, "m": a.m, "shard_bytes": a.shard_bytes, "stripes": 256}
    if a.layout != "pitch":
        cfg["layout"] = a.layout
    erase = sorted(int(x) for x in a.erase.split(","))
    enc, dec, src = bench.load_traffic(a.traffic, {**cfg, "erase": erase})
    assert enc and dec and src == os.path.join("profiles", "hbm_traffic.json")


def test_full_is_off_by_default():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs writes float32 .npy files: an output within DUMP_MAX_VALUES whole, in
    its own shape (a strided view included), a larger one as DUMP_MAX_VALUES of its bytes at
    positions that depend on its shape alone, so two runs sample the same bytes."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    g = torch.Generator().manual_seed(3)
    small = torch.randint(0, 256, (3, 2, 100), dtype=torch.uint8, generator=g)
    big = torch.randint(0, 256, (5, 4, 131), dtype=torch.uint8, generator=g)[:, :, :127]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("small", small), ("big", big)])
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy().astype(np.float32))
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (1000,)
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    # the sample is of big's own bytes: a changed output changes every sampled value
    bench.dump_outputs(str(tmp_path / "c"), [("big", big ^ 0xFF)])
    assert np.array_equal(np.load(tmp_path / "c" / "big.npy"), 255 - b)



@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain bench.py run times its steps and nothing else (no CPU baseline, ceilings or
    layout A/B in the line), and --dump-outputs writes the parity and the rebuilt shards of
    the same seeded batch: the files equal the dump of an encode of that batch made by a
    second process (the rebuilt shards are the data shards the decode erased)."""
    import json
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--stripes",
                        "8", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["metric"] == bench.METRIC
    assert line["cpu_baseline"] is None and "layout_ab" not in line
    assert line["roofline"]["copy_ceiling"] is None and line["roofline"]["frac"] > 0

    # in a process of its own: this one's caching allocator stays untouched, so later tests'
    # batches sit where they did (their plans' address-alignment classes depend on it)
    prog = tmp_path / "want.py"
    prog.write_text(
        "import sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import torch\n"
        "import bench\n"
        "from callfs_amd.device import Plan, StripeBatch\n"
        "sb = StripeBatch(10, 4, 1 << 20, 8, torch.device('cuda:0'), layout='planar')\n"
        "sb.fill_random(0xCA11F5)\n"
        "Plan.for_batch(sb).launch()\n"
        "torch.cuda.synchronize()\n"
        "bench.dump_outputs(sys.argv[1], [('encode_parity', sb.parity()),\n"
        "                                 ('decode_rebuilt', sb.data()[:, :4])])\n")
    r = subprocess.run([sys.executable, str(prog), str(tmp_path / "want")], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("encode_parity", "decode_rebuilt"):
        got, want = np.load(out / (name + ".npy")), np.load(tmp_path / "want" / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == (bench.DUMP_MAX_VALUES,)
        assert np.array_equal(got, want), name


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--decode-into", "inplace"], ["--layout", "pitch"],
                                   ["--split-layout", "readall", "--shard-bytes", "100003"],
                                   ["--split-layout", "--shard-bytes", "100003"],
                                   ["--pitch", str((1 << 20) + 4096)],
                                   ["--object-bytes", str(16 << 20)]])
def test_bench_layouts_run_and_check(extra):
    """bench.py --full end to end on a small batch in every layout it offers: the device
    round trip, the timed steps, the rebuilt-shard check, the ceilings and (planar) the
    in-process pitch / readall layout A/B all pass, and the line parses."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--stripes", "8",
                        "--steps", "3", "--warmup", "1", "--cpu-seconds", "0.5",
                        "--cpu-working-set", str(64 << 20)] + extra,
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["value"] > 0 and line["roofline"]["frac"] > 0
    assert line["cpu_baseline"]["parity_check"].startswith("GPU parity")
    if not extra:
        assert line["config"]["layout"] == "planar"
        ab = line["layout_ab"]
        assert "error" not in ab, ab
        for lay in ("pitch", "readall", "planar"):
            assert 0 < ab[lay]["encode_frac"] < 1 and 0 < ab[lay]["decode_frac"] < 1, lay
