"""Worker of tests/test_qbase_cpu.py's gloo runs (importable so torch.multiprocessing can spawn
it): tests/_dist_worker.py's ``train_worker`` with ``--base_quantization``."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def train_worker(rank, world, port, stage, outdir, kind, micro, steps):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
    import torch

    torch.set_num_threads(1)
    from lumen.lora import adapter_state_dict
    from lumen.models.layers import Linear
    from lumen.parallel.dist import init, shutdown
    from lumen.train.config import load_ds_config
    from lumen.train.trainer import TrainArgs, Trainer

    env = init(device="cpu")
    raw = {"zero_optimization": {"stage": stage, "reduce_bucket_size": 3000},
           "bf16": {"enabled": False}}
    ds = load_ds_config(raw, micro, 1, world, 1e-2, dtype_override="fp32")
    a = TrainArgs(model_name="tiny-llama", synthetic=True, synthetic_samples=64, max_length=16,
                  per_device_train_batch_size=micro, gradient_accumulation_steps=1,
                  max_steps=steps, logging_steps=1, lora_r=4, lora_dropout=0.0,
                  save_strategy="no", save_final=False, output_dir=os.path.join(outdir, "ck"),
                  seed=7, gradient_checkpointing=False, base_quantization=kind)
    t = Trainer(a, ds, env, printer=lambda *x, **k: None)
    t.train()
    if rank == 0:
        nq = sum(1 for m in t.model.modules() if isinstance(m, Linear) and m.qweight is not None)
        torch.save({"sd": adapter_state_dict(t.model),
                    "losses": [r["loss"] for r in t.log_history], "quantized": nq},
                   os.path.join(outdir, f"result_stage{stage}_w{world}.pt"))
    shutdown()
