#!/usr/bin/env python3
"""Flagship training benchmark: GPT-2 345M (hidden 1024, 24 layers, 16 heads,
seq 1024) on synthetic data, bf16, whole-node tokens/s.

Metric/config match BASELINE.json ("tokens/sec (whole node), GPT-2 345M
3D-parallel at 1/2/4/8 MI355X"); the reference numbers are LiBai v0.2.0 fp16
(17.52 samples/s 1n1g ... 125.64 samples/s 1n8g DP8).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
launched via torch.distributed.run with one rank per GPU over RCCL.  W untimed
warmup steps, then exactly K steps bracketed by barrier+synchronize on both
sides, MAX elapsed over ranks, rank 0 prints ONE JSON line.

A plain run does only that.  `--dump-outputs DIR` additionally writes what the
last timed step returned (the loss terms) and a fixed seeded sample of the
parameters it updated as DIR/<name>.npy (float32), so two builds can be
compared output for output: model init, batches and dropout are all seeded.
`--full` is where any secondary measurement belongs (extra precisions, sizes,
baselines); there is none today, so it currently adds nothing to a plain run.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

BASELINE_TOKENS_PER_S = {1: 17.52 * 1024, 2: None, 4: 63.45 * 1024, 8: 125.64 * 1024}


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--micro-batch", type=int, default=None, help="per-rank micro batch")
    p.add_argument("--acc", type=int, default=1, help="grad accumulation steps")
    p.add_argument("--tp", type=int, default=1)
    p.add_argument("--pp", type=int, default=1)
    p.add_argument("--seq-len", type=int, default=1024)
    p.add_argument("--hidden", type=int, default=1024)
    p.add_argument("--layers", type=int, default=24)
    p.add_argument("--heads", type=int, default=16)
    p.add_argument("--vocab", type=int, default=50304)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--act-ckpt", action="store_true")
    p.add_argument("--model", default="gpt2",
                   choices=["gpt2", "bert-large", "llama7b", "llama1b", "vit-l16"],
                   help="flagship benchmark model family")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write the last step's outputs "
                        "to DIR/<name>.npy (float32)")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (none exist yet; "
                        "a plain run measures only the headline figure)")
    return p.parse_args()


def _enable_tuned_gemms():
    """Load the committed hipBLASLt TunableOp algo table (gfx950) if present:
    ~3% on the 345M step, no tuning cost at runtime."""
    table = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libai_amd",
                         "data", "tunableop_gfx950.csv")
    if os.path.exists(table) and "PYTORCH_TUNABLEOP_ENABLED" not in os.environ:
        import shutil
        import tempfile

        # torch inserts the device ordinal before .csv; provide all 8
        d = tempfile.mkdtemp(prefix="tunableop_")
        for i in range(8):
            shutil.copy(table, os.path.join(d, f"tunableop{i}.csv"))
        os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
        os.environ["PYTORCH_TUNABLEOP_TUNING"] = "0"
        os.environ["PYTORCH_TUNABLEOP_FILENAME"] = os.path.join(d, "tunableop.csv")


def build_bench_model(args):
    """Construct the benchmark model for --model; gpt2 honors the shape flags
    (the BASELINE contract); the others are the fixed BASELINE.json configs."""
    if args.model == "gpt2":
        from libai_amd.models import GPTForPreTraining

        m = GPTForPreTraining(
            hidden_layers=args.layers, vocab_size=args.vocab,
            hidden_size=args.hidden, ffn_hidden_size=4 * args.hidden,
            num_attention_heads=args.heads, max_seq_length=args.seq_len,
            embedding_dropout_prob=0.1, attention_dropout_prob=0.1,
            output_dropout_prob=0.1,
        )
        return m, f"gpt2-345m (nl{args.layers} h{args.hidden} nah{args.heads} seq{args.seq_len})"
    if args.model == "bert-large":
        from libai_amd.models import BertForPreTraining

        args.seq_len = 512
        args.vocab = 30592
        args.layers = 24
        m = BertForPreTraining(
            vocab_size=args.vocab, hidden_size=1024, hidden_layers=24,
            num_attention_heads=16, intermediate_size=4096,
            max_position_embeddings=512,
        )
        return m, "bert-large (nl24 h1024 nah16 seq512)"
    if args.model in ("llama7b", "llama1b"):
        from libai_amd.models import LlamaForCausalLM

        if args.model == "llama7b":
            shape = dict(hidden_layers=32, hidden_size=4096, intermediate_size=11008,
                         num_attention_heads=32)
            args.act_ckpt = True  # part of the BASELINE #4 config (7B on 288 GB)
        else:
            shape = dict(hidden_layers=16, hidden_size=2048, intermediate_size=5504,
                         num_attention_heads=16)
        args.seq_len = 2048
        args.vocab = 32000
        args.layers = shape["hidden_layers"]
        m = LlamaForCausalLM(vocab_size=args.vocab,
                             max_position_embeddings=args.seq_len, **shape)
        return m, f"{args.model} (seq2048)"
    if args.model == "vit-l16":
        from libai_amd.models import VisionTransformer

        args.seq_len = 197  # tokens per image (for tokens/s accounting)
        args.layers = 24
        m = VisionTransformer(img_size=224, patch_size=16, embed_dim=1024, depth=24,
                              num_heads=16, num_classes=1000)
        return m, "vit-l16 (224px patch16)"
    raise ValueError(args.model)


def make_batch(args, micro, gen, device):
    if args.model == "vit-l16":
        img = torch.randn(micro, 3, 224, 224, generator=gen)
        lbl = torch.randint(0, 1000, (micro,), generator=gen)
        return {"images": img, "labels": lbl}
    if args.model == "bert-large":
        ids = torch.randint(5, args.vocab, (micro, args.seq_len), generator=gen)
        mask_pos = torch.rand(micro, args.seq_len, generator=gen) < 0.15
        return {
            "input_ids": ids,
            "attention_mask": torch.ones(micro, args.seq_len, dtype=torch.uint8),
            "ns_labels": torch.randint(0, 2, (micro,), generator=gen),
            "lm_labels": ids.clone(),
            "loss_mask": mask_pos.long(),
        }
    toks = torch.randint(0, args.vocab, (micro, args.seq_len + 1), generator=gen)
    return {"input_ids": toks[:, :-1].contiguous(),
            "labels": toks[:, 1:].contiguous()}


DUMP_BUDGET_BYTES = 64 << 20
DUMP_PER_PARAM = 4096


def dump_outputs(out_dir, last_out, model):
    """Write the last timed step's results as float32 .npy files: one
    loss_<name>.npy per returned loss term and params_sample.npy, the same
    seeded element sample of every updated parameter in named_parameters()
    order (at most DUMP_PER_PARAM each, DUMP_BUDGET_BYTES in all)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    if isinstance(last_out, dict):
        for k, v in last_out.items():
            np.save(os.path.join(out_dir, f"loss_{k}.npy"),
                    v.detach().float().cpu().numpy().astype(np.float32))
    elif last_out is not None:
        np.save(os.path.join(out_dir, "loss.npy"),
                torch.as_tensor(last_out).detach().float().cpu().numpy()
                .astype(np.float32))
    params = [p for _, p in model.named_parameters()]
    per = max(1, min(DUMP_PER_PARAM, DUMP_BUDGET_BYTES // 8 // max(len(params), 1)))
    g = torch.Generator().manual_seed(97531)
    parts = []
    for p in params:
        flat = p.detach().reshape(-1)
        if flat.numel() > per:
            idx = torch.randint(0, flat.numel(), (per,), generator=g)
            flat = flat[idx.to(flat.device)]
        parts.append(flat.float().cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"),
            torch.cat(parts).numpy().astype(np.float32))


def main():
    args = parse_args()
    _enable_tuned_gemms()
    world = int(os.environ.get("WORLD_SIZE", 1))
    assert world == args.gpus or world == 1, (
        f"WORLD_SIZE {world} != --gpus {args.gpus}; launch N>1 with torchrun"
    )
    n = max(world, 1)

    from libai_amd.utils import distributed as du

    dutil = du.setup_dist_util(
        dict(
            tensor_parallel_size=args.tp,
            pipeline_parallel_size=args.pp,
            pipeline_num_layers=args.layers,
        )
    )
    rank = dutil.rank
    device = du.get_device()
    if device.type == "cuda":
        torch.cuda.set_device(device)
    torch.manual_seed(1234)  # identical init across DP ranks

    dp = dutil.data_parallel_size
    micro = args.micro_batch
    if micro is None:
        # best-measured per-model micro batch on one MI355X (288 GB)
        per_model = {"gpt2": 48, "bert-large": 96, "llama7b": 12, "llama1b": 8,
                     "vit-l16": 64}
        micro = per_model[args.model] if device.type == "cuda" else 2
    global_batch = micro * dp * args.acc

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if device.type == "cpu" and args.dtype == "bf16":
        dtype = torch.float32  # CPU smoke runs in fp32

    # model: random init at the named benchmark shape
    from libai_amd.optim import FusedAdamW, get_default_optimizer_params

    model, model_name = build_bench_model(args)
    if args.act_ckpt:
        model.set_activation_checkpoint(True)
    model = model.to(dtype)

    pipeline = None
    if args.pp > 1:
        from libai_amd.parallel.pipeline import PipelineScheduler

        model.hidden_size = args.hidden
        pipeline = PipelineScheduler(model, dtype=dtype)
    model = model.to(device)
    model.train()

    optimizer = FusedAdamW(
        get_default_optimizer_params(model, base_lr=1.5e-4, weight_decay=0.01),
        lr=1.5e-4,
        weight_decay=0.01,
        clip_grad=1.0,
    )
    overlap = pipeline is None and optimizer.register_overlap_hooks()

    torch.manual_seed(du.same_seed_for_tp_group(1234))  # diverge dropout per dp rank

    # synthetic batches, pre-generated on host, moved in-step
    gen = torch.Generator().manual_seed(4321 + dutil.data_parallel_rank)
    pool = []
    for _ in range(4):
        b = make_batch(args, micro, gen, device)
        if device.type == "cuda":
            b = {k: (v.pin_memory() if v.is_floating_point() or v.dtype == torch.long
                     or v.dtype == torch.uint8 else v) for k, v in b.items()}
        pool.append(b)

    import torch.distributed as dist

    def to_dev(b):
        return {
            k: (
                v.to(device, dtype=dtype, non_blocking=True)
                if v.is_floating_point()
                else v.to(device, non_blocking=True)
            )
            for k, v in b.items()
        }

    def sync_dp_grads():
        optimizer.grad_sync()

    step_i = 0
    last_out = None  # what the latest step returned to its caller

    def one_step():
        nonlocal step_i, last_out
        if pipeline is not None:
            batches = [to_dev(pool[(step_i * args.acc + j) % len(pool)])
                       for j in range(max(args.acc, 1))]
            last_out = pipeline.run_1f1b(batches)
        else:
            for j in range(args.acc):
                data = to_dev(pool[(step_i * args.acc + j) % len(pool)])
                if overlap and j == args.acc - 1:
                    optimizer.begin_overlap_step()
                losses = model(**data)
                total = sum(v for v in losses.values()) / args.acc
                total.backward()
            last_out = {k: v.detach() for k, v in losses.items()}
        sync_dp_grads()
        optimizer.step()
        optimizer.zero_grad()
        step_i += 1

    def barrier_sync():
        if dist.is_initialized():
            dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_step()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    if dist.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64, device=device
                         if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    tokens = args.steps * global_batch * args.seq_len
    tokens_per_s = tokens / elapsed
    ms_per_step = elapsed / args.steps * 1000
    base = BASELINE_TOKENS_PER_S.get(n) if args.model == "gpt2" else None
    par = f"dp{dp}"
    if args.tp > 1:
        par += f"_tp{args.tp}"
    if args.pp > 1:
        par += f"_pp{args.pp}"

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_out, model)

    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": (
                        "tokens/sec (whole node), GPT-2 345M 3D-parallel at 1/2/4/8 MI355X"
                        if args.model == "gpt2"
                        else f"tokens/sec (whole node), {model_name}"
                    ),
                    "value": round(tokens_per_s, 1),
                    "unit": "tokens/s",
                    "n_gpus": n,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": round(ms_per_step, 2),
                    "higher_is_better": True,
                    "scaling": "weak",
                    "vs_baseline": round(tokens_per_s / base, 2) if base else None,
                    "dtype": args.dtype if device.type == "cuda" else "fp32",
                    "data": "synthetic",
                    "config": {
                        "model": model_name,
                        "global_batch": global_batch,
                        "seq_len": args.seq_len,
                        "parallelism": par,
                    },
                }
            ),
            flush=True,
        )


if __name__ == "__main__":
    main()
