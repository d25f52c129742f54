"""CPU tests for the tooling around the engine: dataset prep, scaling comparison, the launcher,
the Locust profile and LoRA merge/export."""
import csv
import os
import subprocess
import sys
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_format_and_prepare_dataset(tmp_path):
    from lumen.data.prepare import dataset_dir_name, format_conversation_for_llama2

    assert format_conversation_for_llama2({"question": " q? ", "answer": "a."}) == \
        {"text": "<s>[INST] q? [/INST] a.</s>"}
    assert dataset_dir_name(None) == "glaive_code_full"
    assert dataset_dir_name(5000) == "glaive_code_5k"

    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/prepare_dataset.py"),
                          "--num_samples", "2000", "--output_dir", str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    path = tmp_path / "glaive_code_2k"
    from datasets import load_from_disk

    ds = load_from_disk(str(path))
    assert len(ds) == 2000 and ds.column_names == ["text"]
    assert ds[0]["text"].startswith("<s>[INST] ") and ds[0]["text"].endswith("</s>")
    # the training data path reads it back and tokenizes with truncation
    from lumen.data.datasets import build_dataset
    from lumen.data.tokenizer import ByteTokenizer

    tok = ByteTokenizer()
    d = build_dataset(str(path), tok, 64, False, 0, tok.vocab_size)
    assert len(d) == 2000 and max(len(d[i]["input_ids"]) for i in range(20)) <= 64


def test_prepare_from_local_jsonl(tmp_path):
    import json

    from lumen.data.prepare import prepare_dataset

    src = tmp_path / "src.jsonl"
    with open(src, "w") as f:
        for i in range(10):
            f.write(json.dumps({"question": f"q{i}", "answer": f"a{i}"}) + "\n")
    out = prepare_dataset(str(tmp_path / "data"), None, str(src))
    from datasets import load_from_disk

    ds = load_from_disk(out)
    assert ds[3]["text"] == "<s>[INST] q3 [/INST] a3</s>"


def test_compare_training(tmp_path):
    from lumen.utils.compare import compare
    from lumen.utils.metrics import save_training_metrics

    p = str(tmp_path / "m.csv")
    rows = [("baseline", 1, 0, 2.0, 100.0), ("zero2_1gpu", 1, 2, 1.8, 110.0),
            ("zero2_2gpu", 2, 2, 1.0, 200.0), ("zero2_4gpu", 4, 2, 0.6, 330.0)]
    for name, n, st, hours, tok in rows:
        save_training_metrics({"experiment": name, "num_gpus": n, "zero_stage": st,
                               "strategy": "baseline" if st == 0 else f"ZeRO-{st}",
                               "training_time_hours": hours, "samples_per_second": 1.0,
                               "peak_memory_gb": 10.0 / n, "final_loss": 1.0,
                               "tokens_per_second": tok}, p)
    res = compare(p, str(tmp_path / "plots" / "cmp.png"))
    df = res["table"].set_index("experiment")
    assert df.loc["zero2_2gpu", "speedup"] == pytest.approx(2.0)
    assert df.loc["zero2_4gpu", "efficiency"] == pytest.approx(2.0 / 0.6 / 4 * 100)
    assert df.loc["zero2_4gpu", "token_speedup"] == pytest.approx(3.3)
    assert res["plot"] is None or os.path.isfile(res["plot"])
    # CLI without a CSV is a no-op message, not a crash
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/compare_training.py"),
                          "--csv", str(tmp_path / "missing.csv")], capture_output=True, text=True)
    assert out.returncode == 0 and "No metrics" in out.stdout


def _write(path, body):
    path.write_text(textwrap.dedent(body))
    return str(path)


def test_launch_env_and_local_rank(tmp_path):
    script = _write(tmp_path / "w.py", """
        import os, sys, json
        out = sys.argv[1]
        with open(os.path.join(out, "r%s.json" % os.environ["RANK"]), "w") as f:
            json.dump({k: os.environ[k] for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE",
                       "MASTER_ADDR", "MASTER_PORT")} | {"argv": sys.argv[2:]}, f)
        """)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0,1,2")
    out = subprocess.run([sys.executable, "-m", "lumen.launch", "--nproc_per_node", "2",
                          "--master_port", "29555", script, str(tmp_path)], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    import json

    r1 = json.load(open(tmp_path / "r1.json"))
    assert r1["LOCAL_RANK"] == "1" and r1["WORLD_SIZE"] == "2"
    assert r1["MASTER_ADDR"] == "127.0.0.1" and r1["MASTER_PORT"] == "29555"
    assert r1["argv"] == ["--local_rank=1"]


def test_launch_refuses_to_widen_visible_devices(tmp_path):
    script = _write(tmp_path / "w.py", "print('should not run')\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    out = subprocess.run([sys.executable, "-m", "lumen.launch", "--num_gpus", "2", script],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "refusing to widen" in out.stderr
    assert "should not run" not in out.stdout


def test_shared_gpu_rehearsal_mapping(monkeypatch):
    """LUMEN_SHARED_GPU_REHEARSAL: the launcher allows more ranks than GPUs, and dist.init maps
    ranks onto the visible devices round-robin with a per-rank RCCL host id (mocked HIP)."""
    import argparse

    import lumen.parallel.dist as D
    from lumen.launch import build_rank_envs

    a = argparse.Namespace(nproc_per_node=4, num_gpus=None, nnodes=None, node_rank=None,
                           master_addr=None, master_port=29700)
    envs = build_rank_envs(a, {"HIP_VISIBLE_DEVICES": "0", "LUMEN_SHARED_GPU_REHEARSAL": "1"})
    assert [e["LOCAL_RANK"] for e in envs] == ["0", "1", "2", "3"]
    with pytest.raises(SystemExit):
        build_rank_envs(a, {"HIP_VISIBLE_DEVICES": "0"})
    seen = {}
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: seen.setdefault("dev", d))
    monkeypatch.setattr(D.dist, "is_initialized", lambda: False)
    monkeypatch.setattr(D.dist, "init_process_group", lambda **kw: seen.setdefault("kw", kw))
    monkeypatch.setattr(D, "_ENV", None)
    for k, v in dict(RANK="3", WORLD_SIZE="4", LOCAL_RANK="3", LOCAL_WORLD_SIZE="4",
                     LUMEN_SHARED_GPU_REHEARSAL="1").items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("NCCL_HOSTID", raising=False)
    try:
        env = D.init()
        assert env.device == torch.device("cuda", 1) and seen["dev"] == 1
        assert seen["kw"]["backend"] == "nccl" and seen["kw"]["device_id"] == env.device
        assert os.environ["NCCL_HOSTID"] == "lumen-rehearsal-3"
    finally:
        D._ENV = None
        os.environ.pop("NCCL_HOSTID", None)
        os.environ.pop("NCCL_SOCKET_IFNAME", None)


def test_launch_fail_fast(tmp_path):
    script = _write(tmp_path / "w.py", """
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(3)
        time.sleep(300)
        """)
    import time

    t0 = time.time()
    out = subprocess.run([sys.executable, "-m", "lumen.launch", "--nproc_per_node", "2",
                          "--no_local_rank_arg", "--grace", "2", script], cwd=ROOT,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="0,1"), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 3
    assert time.time() - t0 < 60
    assert "rank 1 exited with code 3" in out.stderr


def test_launch_slurm_env():
    from lumen.launch import build_rank_envs, parse_args

    a = parse_args(["--nproc_per_node", "2", "x.py"])
    envs = build_rank_envs(a, {"SLURM_NNODES": "2", "SLURM_NODEID": "1",
                               "SLURM_JOB_NODELIST": "gpu[07-08]", "ROCR_VISIBLE_DEVICES": "0,1"})
    assert [e["RANK"] for e in envs] == ["2", "3"]
    assert envs[0]["WORLD_SIZE"] == "4" and envs[0]["MASTER_ADDR"].startswith("gpu")


def test_locust_payload():
    import random

    from lumen.bench.locustfile import make_payload, parse_sse_line

    b = make_payload(random.Random(0), chat=False, prompt_tokens=8, max_tokens=4)
    assert b["stream"] and b["max_tokens"] == 4 and len(b["prompt"].split()) == 8
    c = make_payload(random.Random(0), chat=True, prompt_tokens=8, max_tokens=4)
    assert c["messages"][0]["role"] == "user"
    assert parse_sse_line(b'data: {"a": 1}') == {"a": 1}
    assert parse_sse_line(b"data: [DONE]") is None and parse_sse_line(b"") is None


def test_merge_lora_export(tmp_path):
    from lumen.lora import LoraConfig, apply_lora, save_adapter
    from lumen.models import build_model

    torch.manual_seed(0)
    m = build_model("tiny-llama", dtype=torch.float32, device=torch.device("cpu"))
    apply_lora(m, LoraConfig(r=4, lora_dropout=0.0))
    for n, p in m.named_parameters():
        if p.requires_grad:
            p.data.normal_(0, 0.05)
    m.eval()
    ids = torch.randint(3, m.config.vocab_size, (2, 12))
    with torch.no_grad():
        ref = m(ids)["logits"] if isinstance(m(ids), dict) else m(ids)
    save_adapter(m, str(tmp_path / "adapter"), "tiny-llama")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/merge_lora.py"), "--model",
                          "tiny-llama", "--adapter", str(tmp_path / "adapter"), "--output_dir",
                          str(tmp_path / "merged"), "--dtype", "fp32"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    merged = build_model(str(tmp_path / "merged"), dtype=torch.float32,
                         device=torch.device("cpu"))
    merged.eval()
    with torch.no_grad():
        got = merged(ids)
        got = got["logits"] if isinstance(got, dict) else got
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


def test_profiler_and_debug_guards(tmp_path, monkeypatch):
    from lumen.parallel.dist import init
    from lumen.train.config import load_ds_config
    from lumen.train.trainer import TrainArgs, Trainer
    from lumen.utils.debug import NonFiniteError, check_finite

    monkeypatch.setenv("LUMEN_PROFILE", "1")
    monkeypatch.setenv("LUMEN_PROFILE_WAIT", "1")
    monkeypatch.setenv("LUMEN_PROFILE_ACTIVE", "2")
    monkeypatch.setenv("LUMEN_PROFILE_DIR", str(tmp_path / "prof"))
    monkeypatch.setenv("LUMEN_DEBUG", "1")
    env = init(device="cpu")
    ds = load_ds_config({"zero_optimization": {"stage": 1}, "wall_clock_breakdown": True}, 2, 1,
                        1, 1e-3, dtype_override="fp32")
    a = TrainArgs(model_name="tiny-llama", synthetic=True, synthetic_samples=16, max_length=16,
                  per_device_train_batch_size=2, max_steps=5, logging_steps=1, lora_r=4,
                  save_strategy="no", output_dir=str(tmp_path / "o"), save_final=False)
    lines = []
    t = Trainer(a, ds, env, printer=lambda *x, **k: lines.append(" ".join(map(str, x))))
    t.train()
    assert os.path.isfile(tmp_path / "prof" / "trace_rank0.json")
    assert any(l.startswith("[lumen] time (ms)") and "fwd" in l for l in lines)
    with pytest.raises(NonFiniteError):
        check_finite("x", torch.tensor([1.0, float("nan")]))


def test_step_watchdog_names_escape_hatch():
    """A rank whose steps stop (hung collective) exits 19 with a message naming
    LUMEN_ZERO3_SHARED_GROUP=1 when ZeRO-3 gathers run on their own communicator; a kicked
    watchdog never fires."""
    code = ("import sys, time, types; sys.path.insert(0, %r)\n"
            "from lumen.utils.debug import StepWatchdog\n"
            "u, e = types.SimpleNamespace(state='inflight'), types.SimpleNamespace(state='empty')\n"
            "c = types.SimpleNamespace(identity=False, units=[u, e, u], schedule='keep', "
            "group=object())\n"
            "ok = StepWatchdog(1.0, 3, c)\n"
            "for _ in range(8):\n    ok.kick(); time.sleep(0.25)\n"
            "ok.close()\nprint('kicked ok', flush=True)\n"
            "StepWatchdog(0.5, 3, c)\ntime.sleep(30)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 19, (r.returncode, r.stderr)
    assert "kicked ok" in r.stdout
    assert "rank 3" in r.stderr and "2 weight gather(s) in flight" in r.stderr
    assert "LUMEN_ZERO3_SHARED_GROUP=1" in r.stderr


def test_concurrent_native_builds(tmp_path):
    """4 processes call ``lumen.csrc.build.build`` on the same fresh build dir at once (what 8
    ranks of a torchrun job do when the extension is missing): the file lock serialises them,
    exactly one links, and the result is one loadable extension with no temp files left.
    The fresh dir is seeded with the big objects of the in-tree build (when present) so the
    test recompiles + links in seconds; every kernel object still has to be current."""
    import shutil

    from lumen.csrc import build as B

    seed_dir = os.path.join(ROOT, "build", "lumen_native")
    bdir = tmp_path / "build"
    bdir.mkdir()
    for name in ("binding.o", "flash_attn.hip.o", "paged_attention.hip.o", "lora_v3.hip.o"):
        if os.path.exists(os.path.join(seed_dir, name)):
            shutil.copy2(os.path.join(seed_dir, name), bdir / name)
    out = tmp_path / "ext" / "_C.so"
    code = ("import sys; sys.path.insert(0, %r); from lumen.csrc.build import build; "
            "build(jobs=2, build_dir=%r, out=%r)" % (ROOT, str(bdir), str(out)))
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for _ in range(4)]
    logs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-3000:]
    assert sum(l.count("[lumen.build] linked") for l in logs) == 1, logs
    assert not [f for f in os.listdir(out.parent) if ".part" in f]
    assert not [f for f in os.listdir(bdir) if ".part" in f]
    chk = ("import importlib.util as u, sys; import torch; s = u.spec_from_file_location('_C', %r);"
           " m = u.module_from_spec(s); s.loader.exec_module(m); print('ok', len(dir(m)))"
           % str(out))
    r = subprocess.run([sys.executable, "-c", chk], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stderr[-2000:]
    assert B.ext_path().endswith(".so")


@pytest.mark.parametrize("world", [2, 4, 8])
def test_bench_contract_torchrun(world):
    """bench.py under torch.distributed.run (2 / 4 ranks, gloo, tiny model): one JSON line from
    rank 0 with the driver's fields, whole-job tokens/s, ZeRO-3 partitioning active on its own
    gather communicator, and the comm diagnostics (collective-observed world size, gathered /
    received bytes, exposed gather wait, peak memory over ranks)."""
    import json
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port",
                          str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(world),
                          "--steps", "2", "--warmup", "1", "--model", "tiny-llama", "--seq_len",
                          "32", "--micro_batch", "2", "--partitioned_steps", "2", "--full"],
                         capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    # the driver contract: rank 0's stdout is exactly that one JSON line (logs go to stderr)
    assert [l for l in out.stdout.splitlines() if l.strip()] == lines, out.stdout[-2000:]
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in j, k
    assert j["n_gpus"] == world and j["steps"] == 2 and j["scaling"] == "weak"
    assert j["config"]["global_batch"] == 2 * world
    assert j["config"]["parallelism"].startswith(f"dp{world}-zero3-keep")
    x = j["extra"]
    # the partitioned schedules, timed after the headline region on fresh engines
    for sched in ("release", "hybrid"):
        p = x[f"zero3_{sched}"]
        assert p["schedule"] == sched and p["ms_per_step"] > 0, p
        assert p["gathered_mb_per_step"] > 0 and p["steps"] == 2, p
    assert x["zero3_release"]["stage3_max_live_parameters"] == int(1e9)
    # "auto" live budget: one gathered copy, gathered once (warm-up) and kept resident
    assert x["zero3"]["schedule"] == "keep", x["zero3"]
    # keep gathers once, on the default communicator (no second RCCL communicator per GPU)
    assert not x["zero3"]["separate_group"] and x["zero3"]["reason"]
    assert x["rccl_world"] == world and x["gather_group_world"] is None
    assert x["zero3_gathered_mb_total"] > 0
    assert x["zero3_gathered_mb_per_step"] == 0 and x["zero3_received_mb_per_step_per_rank"] == 0
    assert x["zero3_exposed_wait_ms_per_step_max_rank"] >= 0
    assert "peak_hbm_gb_max_rank" in x and x["setup_s"] > 0
    tokens = 2 * world * 32 * 2
    assert abs(j["value"] - tokens / (j["ms_per_step"] * 2 / 1000)) / j["value"] < 0.02
    # transport self-diagnosis (VERDICT r4 Next #4): probe numbers and the link time each
    # partitioned schedule's gather volume implies at the probe's bus bandwidth
    c = x["comm"]
    assert c["world"] == world and c["all_gather"]["busbw_gbps"] > 0, c
    assert c["all_gather"]["busbw_gbps"] == pytest.approx(
        c["all_gather"]["algbw_gbps"] * (world - 1) / world, rel=0.05, abs=0.11)
    assert c["reduce_scatter"]["ms"] > 0 and c["reduce_scatter"]["numel"] > 0
    for sched in ("release", "hybrid"):
        p = x[f"zero3_{sched}"]
        assert p["probe_busbw_gbps"] == c["all_gather"]["busbw_gbps"]
        assert p["implied_link_ms_per_step"] > 0


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain bench.py run (no --full; CPU, tiny model) times exactly --steps steps, prints the
    one result line with the driver's fields and none of the sections that --full adds, and
    --dump-outputs writes the last step's outputs as float32 / float64 .npy files that a second
    run with the same arguments reproduces (same seeded inputs; CPU sums are ordered)."""
    import json

    import numpy as np

    def run(d):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                              "--steps", "3", "--warmup", "1", "--model", "tiny-llama",
                              "--seq_len", "32", "--micro_batch", "2", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, OMP_NUM_THREADS="2"))
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-2000:]
        return json.loads(lines[0])

    j = run(tmp_path / "a")
    run(tmp_path / "b")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0
    assert abs(j["value"] - 2 * 32 / (j["ms_per_step"] / 1000)) / j["value"] < 0.02
    x = j["extra"]
    assert x["serve"] is None and x["comm"] is None and x["box"] is None
    assert "zero3_release" not in x and "zero3_hybrid" not in x and "serve_tp" not in x
    assert x["budget"]["ran"] == [] and x["budget"]["skipped"] == []
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["adapter_norms.npy", "adapter_sample.npy", "loss.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 * 2**20
    assert np.load(tmp_path / "a" / "loss.npy")[0] == pytest.approx(x["final_loss"], abs=1e-4)
    assert np.load(tmp_path / "a" / "adapter_sample.npy").size == j["config"]["trainable_params"]
    assert (np.load(tmp_path / "a" / "adapter_norms.npy") > 0).all()


def test_gemm_wave_split_plan():
    """Whole-wave column split of the training and serving-prefill GEMMs (lumen/ops/gemm.py):
    only where the last wave of 256x256 tiles on 256 CUs is at most 3/4 full, at a column-tile
    boundary (taken at run time only where both parts are in the tuned table)."""
    from lumen.ops.gemm import mm_nt, split_cols

    assert split_cols(4096, 22016) == 20480      # gate|up fwd: 1376 tiles -> 1280 + 96
    assert split_cols(1024, 22016) == 16384      # 344 tiles -> 256 + 88
    assert split_cols(2048, 12288) == 8192       # serving mixed step q|k|v: 384 -> 256 + 128
    assert split_cols(2048, 22016) == 16384      # serving mixed step gate|up: 688 -> 512 + 176
    for M, N in [(4096, 4096), (4096, 12288), (4096, 32000), (4000, 22016), (256, 1024)]:
        assert split_cols(M, N) == 0, (M, N)     # whole waves, >3/4-full tail, or ragged M
    x, w = torch.randn(8, 16), torch.randn(24, 16)
    assert torch.allclose(mm_nt(x, w), x @ w.t())  # CPU: plain matmul


def test_decode_gemm_plan_table_loads():
    """The shipped decode-GEMM plan table (configs/kernels/, outside the DeepSpeed config glob)
    parses into (N, K, BM) -> (BN, split-K, waves) entries the serving projections look up."""
    from lumen.ops import gemm

    gemm._dg_plans = None
    plans = gemm.dg_plans()
    assert plans, "configs/kernels/decode_gemm_plans.json missing or empty"
    for (n, k, bm), (bn, s, nw) in plans.items():
        assert k % 64 == 0 and bm in gemm.DG_BMS and nw in (4, 8) and 1 <= s <= k // 64


def test_plan_getters_share_one_reader(tmp_path, monkeypatch):
    """The five ``*_plans()`` getters honour their environment override and give {} for a missing
    file; ``dg_plans()`` fills in 4 waves where an entry has no ``NW``; the ``load_*_plans`` names
    parse one file to one dictionary."""
    import json

    from lumen.ops import gemm

    path = tmp_path / "plans.json"
    path.write_text(json.dumps({"plans": [{"N": 4096, "K": 4096, "BM": 64, "BN": 128, "S": 2},
                                          {"N": 512, "K": 256, "BM": 256, "BN": 64, "S": 1,
                                           "NW": 8}]}))
    want = {(4096, 4096, 64): (128, 2), (512, 256, 256): (64, 1)}
    loaders = (gemm.load_w8_plans, gemm.load_w8a8_plans, gemm.load_w4a8_plans,
               gemm.load_w4a16_plans)
    for load in loaders:
        assert load(str(path)) == want
        assert load(str(tmp_path / "missing.json")) == {}
    getters = {"LUMEN_DGEMM_PLANS": ("_dg_plans", gemm.dg_plans),
               "LUMEN_W8_PLANS": ("_w8_plans", gemm.w8_plans),
               "LUMEN_W8A8_PLANS": ("_w8a8_plans", gemm.w8a8_plans),
               "LUMEN_W4A8_PLANS": ("_w4a8_plans", gemm.w4a8_plans),
               "LUMEN_W4A16_PLANS": ("_w4a16_plans", gemm.w4a16_plans)}
    for env, (cache, get) in getters.items():
        monkeypatch.setenv(env, str(path))
        monkeypatch.setattr(gemm, cache, None)
        if get is gemm.dg_plans:
            assert get() == {(4096, 4096, 64): (128, 2, 4), (512, 256, 256): (64, 1, 8)}
        else:
            assert get() == want, env
        assert getattr(gemm, cache) is get()          # cached in the getter's own global
        monkeypatch.setenv(env, str(tmp_path / "missing.json"))
        monkeypatch.setattr(gemm, cache, None)
        assert get() == {}, env
        monkeypatch.setattr(gemm, cache, None)        # the next user reloads the shipped table


@pytest.mark.parametrize("deadline", [300.0, 0.01])
def test_bench_tp_serving_section_and_deadline(deadline):
    """bench.py's TP = N serving section (forced on gloo with --serve_tp 2, tiny model, 8
    requests): with time to finish, rank 0's single JSON line carries extra.serve_tp from the
    TP = 2 engine; with a deadline the section cannot meet, the line still comes out, once,
    with extra.serve_tp = the timeout, and every rank exits 0."""
    import json
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                          str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2",
                          "--steps", "1", "--warmup", "1", "--model", "tiny-llama-gqa",
                          "--seq_len", "32", "--micro_batch", "2", "--partitioned", "",
                          "--serve_tp", "2", "--serve_tp_shape", "8,24,6",
                          "--serve_tp_deadline", str(deadline), "--full"],
                         capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    stp = json.loads(lines[0])["extra"]["serve_tp"]
    if deadline > 100:
        assert stp["output_tokens"] == 8 * 6 and stp["config"]["tp"] == 2, stp
    else:
        assert "timed out" in stp["error"], stp


def test_custom_allreduce_crossover_selection():
    """pick_plan (lumen/parallel/custom_ar.py): the measured one-/two-shot crossover and the
    size from which RCCL takes eager calls (VERDICT r4 Next #4: replaces guessed constants)."""
    from lumen.parallel.custom_ar import pick_plan

    KB, MB = 1 << 10, 1 << 20
    t = [dict(bytes=8 * KB, one=9, two=14, rccl=30), dict(bytes=256 * KB, one=20, two=21, rccl=40),
         dict(bytes=512 * KB, one=35, two=26, rccl=41), dict(bytes=2 * MB, one=90, two=60, rccl=70),
         dict(bytes=8 * MB, one=300, two=200, rccl=120)]
    p = pick_plan(t)
    # two-shot first wins (by > 3 %) at 512 KiB -> one-shot up to 256 KiB; RCCL only at 8 MiB
    assert p == {"one_shot_max": 256 * KB, "rccl_from": 8 * MB}
    # within the noise margin one-shot keeps the size; RCCL must win at every larger size too
    t2 = [dict(bytes=8 * KB, one=10, two=9.8, rccl=9), dict(bytes=1 * MB, one=40, two=30, rccl=50),
          dict(bytes=4 * MB, one=100, two=80, rccl=70)]
    p2 = pick_plan(t2)
    assert p2["one_shot_max"] == 8 * KB and p2["rccl_from"] == 4 * MB
    # one-shot never loses, RCCL never wins; no RCCL column at all
    t3 = [dict(bytes=8 * KB, one=5, two=9), dict(bytes=64 * KB, one=8, two=12)]
    assert pick_plan(t3) == {"one_shot_max": 64 * KB, "rccl_from": None}
    # two-shot wins from the smallest size
    assert pick_plan([dict(bytes=8 * KB, one=20, two=10)])["one_shot_max"] == 0


def test_overlap_mlp_plan_cpu_is_off():
    """The side-stream MLP (``_OverlapMLP``) never plans on CPU tensors; the unfused path runs."""
    import torch

    from lumen.models.layers import Linear
    from lumen.ops.activation import overlap_mlp_plan

    gu, dn = Linear(64, 2 * 96), Linear(96, 64)
    assert overlap_mlp_plan(torch.randn(8, 64), gu, dn) == 0


def test_overlap_bucket_cap():
    """The overlapped ZeRO-2/3 gradient buckets (opt-in LUMEN_DP_BUCKET_MB): the LoRA set of
    Llama-2-7B (16.8 M fp32 elements, one 5e7 DeepSpeed bucket) splits into 16 MiB buckets at
    world > 1, so all but the last reduce-scatter run under the backward; world 1,
    non-overlapped stages and a cap of 0 (the default) keep the config's size."""
    from lumen.parallel.zero import overlap_bucket_numel

    assert overlap_bucket_numel(int(5e7), 8, True, 16) == 4 * 2**20
    assert -(-16_777_216 // overlap_bucket_numel(int(5e7), 8, True, 16)) == 4
    assert overlap_bucket_numel(3000, 8, True, 16) == 3000      # already smaller
    assert overlap_bucket_numel(int(5e7), 1, True, 16) == int(5e7)
    assert overlap_bucket_numel(int(5e7), 8, False, 16) == int(5e7)
    assert overlap_bucket_numel(int(5e7), 8, True, 0) == int(5e7)
    assert overlap_bucket_numel(int(5e7), 8, True) == int(5e7)  # default: off


def test_wall_budget_logic():
    """lumen/bench/budget.py: sections run while their estimate fits in what is left of one
    overall deadline (agreed as the minimum over ranks), and skipped ones are recorded."""
    from lumen.bench.budget import WallBudget, partitioned_estimate_s

    now = [100.0]
    agreed = []

    def agree(x):  # a slower peer: the minimum over ranks is what counts
        agreed.append(x)
        return x - 5.0

    b = WallBudget(60.0, 100.0, agree, clock=lambda: now[0])
    assert b.allow("comm_probe", 30.0)           # left 60 -> agreed 55
    now[0] += 12.0
    b.done("comm_probe")
    assert not b.allow("zero3_release", 50.0)    # left 48 -> agreed 43 < 50
    assert b.allow("zero3_hybrid", 40.0)
    now[0] += 3.0
    b.done("zero3_hybrid")
    r = b.record()
    assert [x["section"] for x in r["ran"]] == ["comm_probe", "zero3_hybrid"]
    assert r["ran"][0]["took_s"] == 12.0 and r["ran"][0]["left_s"] == 55.0
    assert r["skipped"] == [{"section": "zero3_release", "est_s": 50.0, "left_s": 43.0}]
    assert r["left_at_record_s"] == 45.0 and agreed == [60.0, 48.0, 48.0]
    assert partitioned_estimate_s(90.0, 5, 2, 1.0) == pytest.approx(10 + 2 + 7 * 0.09 * 1.5)


def test_bench_wall_budget_skips_sections_torchrun():
    """bench.py at world 2 (gloo, tiny model) with a wall budget already spent by the headline:
    the comm probe and both partitioned schedules are skipped on every rank alike (no
    collective mismatch), the record lists them, and rank 0 still prints its one JSON line."""
    import json
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                          str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2",
                          "--steps", "1", "--warmup", "1", "--model", "tiny-llama", "--seq_len",
                          "32", "--micro_batch", "2", "--wall_budget", "1", "--full"],
                         capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    x = json.loads(lines[0])["extra"]
    skipped = {d["section"] for d in x["budget"]["skipped"]}
    assert {"comm_probe", "zero3_release", "zero3_hybrid"} <= skipped, x["budget"]
    assert x["comm"] is None and x["zero3_release"]["skipped"] == "wall budget"
    assert x["budget"]["ran"] == [] and x["budget"]["wall_budget_s"] == 1.0


def test_box_hwmon_sampler_reads_fake_sysfs(tmp_path):
    """extra.box's clock / power sampler (lumen/utils/boxcal.py) on a fake hwmon directory:
    SCLK from freq1_input (Hz), power from power1_average (uW), summarised as mean / min / p50 /
    max; a missing hwmon (CPU runs, containers without sysfs) yields an empty record, no thread."""
    import time as _time

    from lumen.utils.boxcal import HwmonSampler, gpu_hwmon, summarize

    hw = tmp_path / "hwmon7"
    hw.mkdir()
    (hw / "freq1_input").write_text("1900000000\n")
    (hw / "power1_average").write_text("1350000000\n")
    smp = HwmonSampler(str(hw), period_s=0.002).start()
    _time.sleep(0.05)
    (hw / "freq1_input").write_text("2000000000\n")
    _time.sleep(0.05)
    rec = smp.stop()
    assert rec["hwmon"] == str(hw) and rec["samples"] >= 4
    assert rec["sclk_mhz_min"] == 1900.0 and rec["sclk_mhz_max"] == 2000.0
    assert 1900.0 <= rec["sclk_mhz_mean"] <= 2000.0
    assert rec["power_w_mean"] == 1350.0 and rec["power_w_max"] == 1350.0
    # no hwmon: nothing sampled, no thread started
    none = HwmonSampler(None).start()
    assert none._t is None and none.stop() == {"hwmon": None, "samples": 0}
    s = summarize([3.0, 1.0, 2.0], [], "x")
    assert (s["sclk_mhz_min"], s["sclk_mhz_p50"], s["sclk_mhz_max"]) == (1.0, 2.0, 3.0)
    assert "power_w_mean" not in s
    # CPU: no device properties -> no hwmon path
    assert gpu_hwmon() is None
