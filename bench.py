#!/usr/bin/env python3
"""Headline benchmark: output tokens/s + p50 TTFT of /v1/chat/completions serving, Llama-3-8B-Instruct
Q4_K_M, one serving replica per GPU (BASELINE.json config #2; N GPUs = N data-parallel replicas).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 it is launched with
torch.distributed.run, one rank per GPU (RCCL) — or, called without a torchrun environment, bench.py starts
torch.distributed.run itself as a child process with N ranks (spawn_ranks). Every rank checks world == N.
BASELINE config #3 (Llama-3-70B Q4_K_M, TP=8 over xGMI): `python bench.py --gpus 8 --tp 8 --model llama3-70b`.
Each rank:
  * builds a random-init Llama-3-8B with the exact Q4_K_M tensor types of a real checkpoint
    (models/synthetic.py; no network for weights) and its LLM engine (paged KV, continuous batching,
    hipGraph decode) inside an LLM gRPC worker (workers/llm.py, grpc.aio server) in this process;
  * (`--path http`, default) starts the HTTP gateway (`python -m localai_tfp_amd run`, FastAPI) in a
    child process, pointed at the worker as an external gRPC backend, and a closed-loop load generator
    (tools/loadgen.py) in another child: `--concurrency` users streaming chat completions
    (prompt `--prompt-len` tokens after the Llama-3 chat template, `--gen-len` tokens, ignore_eos);
  * (`--path engine`) drives the engine directly in-process (kernel/scheduler-only number).
A bench "step" is a fixed group of G = --step-group (default 16) engine iterations (one engine iteration =
one continuous-batching forward: every running sequence's decode row + chunked prefill of arriving prompts).
One engine iteration at c128 takes ~5-11 ms and a 256-token generation takes 256 of them, so a 20-iteration
window sees either no prefill at all or a burst of it (VERDICT r5 Weak #1); 20 grouped steps = 320 iterations
cover more than one full generation, i.e. the stationary mix of decode rows, prompt chunks and completions.
The engine thread itself brackets the window: after W*G iterations of the steady state it does device sync +
barrier and records t0, after K*G more again sync + barrier and t1, so exactly K steps (K*G iterations) are timed
on every rank. Output tokens = tokens the engine generated inside the window; TTFT = client-side time from
sending the request to the first content chunk, over requests whose first token arrived inside the window.
The JSON reports the window's engine iterations, prompt (prefill) tokens, output tokens and TTFT sample count.
value = sum over ranks of tokens / max over ranks of window. Rank 0 prints one JSON line.

A plain run does what that line needs and no more: load, tune, capture, one load phase with the reference's
sampling defaults, the window. `--full` adds the rest: a second load phase with greedy sampling on the same
server (`config.other_phases`), and rank 0 exits 3 when fewer than 32 TTFT samples fell in the window (a
window that timed no prefill; a plain run only warns). `--dump-outputs DIR` writes DIR/logits.npy after the
timed steps (dump_outputs below).
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import subprocess
import sys
import tempfile
import threading
import time

T_PROC = time.time()  # before the heavy imports: config.timeline_s counts from here

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "output tokens/sec + p50 TTFT, /v1/chat/completions Llama-3-8B Q4_K at 1/2/4/8 MI355X"
TEMPLATE_OVERHEAD = 24  # Llama-3 chat template tokens around one user message (ByteTokenizer)
TIMELINE: dict = {}  # seconds since process start at which each part of the run was over (config.timeline_s)


def mark(name: str):
    TIMELINE[name] = round(time.time() - T_PROC, 2)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=25, help="timed bench steps (each = --step-group engine iterations)")
    ap.add_argument("--warmup", type=int, default=10, help="untimed bench steps after the steady-state gate")
    ap.add_argument("--step-group", type=int, default=16,
                    help="engine iterations per bench step (G): K steps time K*G continuous-batching iterations")
    ap.add_argument("--min-ttft-samples", type=int, default=32,
                    help="rank 0 warns (with --full: exits non-zero) if fewer TTFT samples fall in the window "
                         "(0: no check)")
    ap.add_argument("--model", default="llama3-8b", choices=["llama3-8b", "llama3-70b", "llama32-1b", "qwen3-30b-a3b", "qwen3-8b"],
                    help="qwen3-30b-a3b: the gallery's first entry (128 experts, 8 active) on the MoE path")
    ap.add_argument("--path", default="http", choices=["http", "engine"])
    ap.add_argument("--ftype", default="Q4_K_M", choices=["Q4_K_M", "Q3_K_M"],
                    help="block-format mix of the synthetic checkpoint (the headline config is Q4_K_M)")
    ap.add_argument("--concurrency", type=int, default=128)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--gen-len", type=int, default=256)
    ap.add_argument("--max-batched-tokens", type=int, default=416,
                    help="tokens per engine step (the engine default: a c128 decode batch + a 288-token prompt chunk)")
    ap.add_argument("--prefill-chunk", type=int, default=0, help="prompt tokens per sequence per step (0: budget)")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--dp-gateway", default="per-rank", choices=["per-rank", "single"],
                    help="http path under DP: one gateway + load generator per rank, or ONE `local-ai run` gateway "
                         "(--gateway-workers processes) in front of every rank's worker, as `data_parallel: N` is "
                         "deployed")
    ap.add_argument("--gateway-workers", type=int, default=0, help="single gateway's processes (0: one per GPU)")
    ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "f16", "fp8"],
                    help="paged KV cache element type (llama.cpp cache_type_k/v); fp8 = e4m3")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--steady-finished", type=int, default=-1,
                    help="completed requests before the warmup count starts (-1: 2 x concurrency)")
    ap.add_argument("--timeout", type=float, default=900.0, help="abort if the window is not reached")
    ap.add_argument("--tp", type=int, default=1,
                    help="tensor-parallel ranks per serving replica (BASELINE config #3: --model llama3-70b "
                         "--gpus 8 --tp 8); world = dp x tp, rank 0 of every group leads")
    ap.add_argument("--no-tp-check", action="store_true", help="skip the TP-vs-unsharded logits self-check")
    ap.add_argument("--tp-rehearsal", type=int, default=0,
                    help="one process runs rank 0's shard of a TP=N model with the collectives as no-ops: the "
                         "per-GPU compute of a TP step on one GPU (config #3 readiness; communication excluded)")
    ap.add_argument("--tokenizer", default="bpe", choices=["bpe", "byte"],
                    help="bpe: a synthetic Llama-3-sized byte-level BPE vocabulary (128,256 ids, tokenizer/synth_bpe.py) "
                         "served through the GGUF BPE tokenizer; byte: one token per byte (no detokenisation work)")
    ap.add_argument("--phases", default=None,
                    help="comma list of sampling phases measured back to back on the same server: reference = "
                         "the reference's defaults (temperature 0.9, top_k 40, top_p 0.95; backend_config.go "
                         "SetDefaults) on the GPU sampler; greedy = argmax. The first phase is the headline "
                         "(default: reference; with --full: reference,greedy)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the greedy phase after the headline phase (HTTP "
                         "path) and the exit status 3 for a window with fewer than --min-ttft-samples TTFT samples")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the probe batch's logits to DIR/logits.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.phases is None:
        args.phases = "reference,greedy" if args.full else "reference"
    if args.dump_outputs and args.tp > 1:
        raise SystemExit("--dump-outputs runs on one rank's engine (no --tp)")
    if args.dump_outputs and args.phases.split(",")[0] == "greedy":
        raise SystemExit("--dump-outputs records the logits the sampler receives; a greedy headline phase takes its "
                         "ids from the step's argmax head instead (see dump_outputs)")
    return args


SAMPLING = {"reference": {"temperature": 0.9, "top_k": 40, "top_p": 0.95},
            "greedy": {"temperature": 0.0},
            # the reference defaults plus a repetition penalty / a JSON-mode grammar (HTTP path only): requests
            # that need host state per token stay on the overlap pipeline
            "penalty": {"temperature": 0.9, "top_k": 40, "top_p": 0.95, "frequency_penalty": 0.5},
            "json": {"temperature": 0.9, "top_k": 40, "top_p": 0.95, "json": True}}


def make_tokenizer(kind: str, vocab: int):
    from localai_tfp_amd.tokenizer import ByteTokenizer
    if kind == "byte":
        return ByteTokenizer(vocab)
    from localai_tfp_amd.tokenizer.synth_bpe import llama3_like_tokenizer
    tok = llama3_like_tokenizer()
    if tok.vocab_size != vocab:
        raise SystemExit(f"synthetic BPE vocabulary has {tok.vocab_size} ids, the model {vocab}")
    return tok


def prompt_sizing(tok, prompt_len: int):
    """(template tokens, words of the load generator's vocabulary per prompt) so that a chat request's
    prompt is ~prompt_len tokens after the chat template."""
    from localai_tfp_amd.templates.chat import render_chat
    from localai_tfp_amd.tools.loadgen import WORDS
    overhead = len(tok.encode(render_chat([{"role": "user", "content": ""}], tok)))
    rng = np.random.default_rng(0)
    sample = " ".join(rng.choice(WORDS, size=2000))
    per_word = len(tok.encode(sample, add_special=False)) / 2000.0
    return overhead, max(1, int(round((prompt_len - overhead) / per_word)))


def generated_ahead(src, workers: int = 8):
    """The synthetic source with every tensor drawn ahead of the loader on a thread pool (numpy's generators
    release the GIL). Each tensor's bytes depend on its name and the seed alone, so the model is the same; the
    load no longer waits for one core to draw 5 GB of random blocks between its uploads."""
    import concurrent.futures as cf
    last = "token_embd.weight"  # first in the plan, read last by the loader
    names = [n for n in src.plan if n != last] + [n for n in src.plan if n == last]
    ex = cf.ThreadPoolExecutor(workers)
    ahead = {n: ex.submit(src, n) for n in names}
    ex.shutdown(wait=False)

    def get_tensor(name):
        f = ahead.pop(name, None)
        return f.result() if f is not None else src(name)

    get_tensor.plan = src.plan
    return get_tensor


def prompt_maker(args, tok, rng):
    """() -> token ids of one chat request (~--prompt-len tokens after the chat template), drawn from `rng`."""
    from localai_tfp_amd.templates.chat import render_chat
    from localai_tfp_amd.tools.loadgen import WORDS as words
    n_words = None if args.tokenizer == "byte" else prompt_sizing(tok, args.prompt_len)[1]

    def make_prompt():
        if n_words is None:
            body = " ".join(rng.choice(words, size=args.prompt_len))[: max(1, args.prompt_len - TEMPLATE_OVERHEAD)]
        else:
            body = " ".join(rng.choice(words, size=n_words))
        return tok.encode(render_chat([{"role": "user", "content": body}], tok))

    return make_prompt


DUMP_COLUMNS = 8192  # vocabulary columns kept per row (a fixed seeded sample: 128 rows x 8192 x fp32 = 4 MB)


def dump_outputs(args, eng, tok, phase, out_dir):
    """--dump-outputs: what the timed path computes for a fixed batch, as DIR/logits.npy (float32).

    The rows of the window's own last step are whichever requests the closed-loop clients had in flight at
    that moment, so they differ from run to run. Once the timed steps are over, the same engine (weights, tuned
    GEMM plans, step graphs, sampler of the headline phase) therefore serves one more batch that is the same in
    every run: --concurrency chat prompts from a fixed seed, submitted together, one token each. The engine
    steps through them exactly as it stepped inside the window (continuous batching, chunked prefill), and the
    logits row each request's token is sampled from, as the sampler receives it, is kept: logits.npy is
    [request, column] over a fixed seeded sample of DUMP_COLUMNS vocabulary columns. Logits rather than
    the sampled ids: at temperature 0.9 an id flips on a last-bit difference of its row, which no tolerance
    covers. A greedy headline phase takes its ids from the step's argmax head and never hands logits to the
    sampler: nothing could be recorded then, so such a run is refused when it starts."""
    from localai_tfp_amd.engine.sequence import Request
    from localai_tfp_amd.ops.sampling import SamplingParams
    for rid in list(eng.seqs):  # engine path: the requests still running when the window closed
        eng.abort(rid)
    eng.run_until_done()
    make_prompt = prompt_maker(args, tok, np.random.default_rng(4321))
    n, V = args.concurrency, eng.model.cfg.vocab
    cols = np.sort(np.random.default_rng(99).choice(V, size=min(V, DUMP_COLUMNS), replace=False))
    cols_dev = torch.from_numpy(cols).to(eng.device)
    logits = np.zeros((n, len(cols)), np.float32)
    row_of, seen = {}, set()
    sample = eng.sampler.sample

    def tap(lg, params, histories, steps, *a, **kw):
        rows = lg[:len(params)].index_select(1, cols_dev).float().cpu().numpy()  # before the sampler edits lg
        for r, p in enumerate(params):
            i = row_of.get(id(p))
            if i is not None and steps[r] == 0:
                logits[i] = rows[r]
                seen.add(i)
        return sample(lg, params, histories, steps, *a, **kw)

    sp = {k: v for k, v in SAMPLING[phase].items() if k != "json"}
    # no prefix reuse: every probe row is computed in this batch, not taken from the KV blocks an earlier request left
    reqs = [Request(make_prompt(), SamplingParams(**sp, ignore_eos=True), max_tokens=1, cache_prompt=False)
            for _ in range(n)]
    row_of.update({id(r.params): i for i, r in enumerate(reqs)})
    eng.sampler.sample = tap
    try:
        for r in reqs:
            eng.submit(r)
        eng.run_until_done()
    finally:
        del eng.sampler.sample
    if len(seen) != n:
        raise SystemExit(f"--dump-outputs: the sampler saw {len(seen)} of {n} probe rows (phase {phase})")
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "logits.npy"), logits)


class _GroupSync:
    """dist-like facade whose barrier / all_reduce run on one process group (the replica leaders)."""

    def __init__(self, dist, group):
        self.dist, self.group = dist, group
        self.ReduceOp = dist.ReduceOp

    def barrier(self):
        self.dist.barrier(group=self.group)

    def all_reduce(self, t, op=None):
        self.dist.all_reduce(t, op=op if op is not None else self.dist.ReduceOp.SUM, group=self.group)


def setup_tp(args, world, rank, dev):
    """world = dp x tp: RCCL group per replica (model all-reduces), two gloo groups per replica (plan
    channel + collectives, parallel/tp_engine.py), and a leaders group for the bench's barriers."""
    import torch.distributed as dist
    from localai_tfp_amd.parallel.tp_engine import TPLink, tp_timeout
    tp = args.tp
    if world % tp:
        raise SystemExit(f"--tp {tp} does not divide world size {world}")
    dp = world // tp
    mine = None
    for g in range(dp):
        ranks = list(range(g * tp, (g + 1) * tp))
        gpu = dist.new_group(ranks)
        cpu = dist.new_group(ranks, backend="gloo", timeout=tp_timeout())
        sync = dist.new_group(ranks, backend="gloo", timeout=tp_timeout())
        if rank in ranks:
            mine = (g, gpu, cpu, sync, ranks[0])
    leaders = dist.new_group([g * tp for g in range(dp)])
    g, gpu, cpu, sync, src = mine
    link = TPLink(rank % tp, tp, cpu, gpu, src=src, sync_group=sync)
    return link, gpu, (_GroupSync(dist, leaders) if dp > 1 else None), dp


def free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def wait_http(url: str, timeout: float, proc=None):
    import urllib.request
    t0 = time.time()
    while time.time() - t0 < timeout:
        if proc is not None and proc.poll() is not None:
            raise RuntimeError(f"gateway exited with {proc.returncode}")
        try:
            with urllib.request.urlopen(url, timeout=2) as r:
                if r.status == 200:
                    return
        except Exception:
            time.sleep(0.25)
    raise TimeoutError(url)


def spawn_ranks(args) -> int | None:
    """`--gpus N` (N > 1) without a torchrun environment: start N ranks as CHILD processes of
    torch.distributed.run (never exec: this process has not touched the GPU, but the children will), pass the
    rank-0 JSON line through (inherited stdout) and return their exit code. None: already a rank / one GPU."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return None
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL / CUDA-tensor sharing across ranks)
    p = subprocess.run(cmd, env=env)
    return p.returncode


def main():
    args = parse()
    rc = spawn_ranks(args)
    if rc is not None:
        sys.exit(rc)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the torchrun world has {world} ranks")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:  # CPU rehearsal of the multi-rank paths (gloo)
            dist.init_process_group("gloo")
    dev = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda":
        torch.cuda.set_device(dev)

    from localai_tfp_amd import _build
    _build.build_all()
    from localai_tfp_amd.engine.engine import EngineConfig, LLMEngine
    from localai_tfp_amd.models import config as C
    from localai_tfp_amd.models.llama import LlamaModel
    from localai_tfp_amd.models.synthetic import synthetic_source
    from localai_tfp_amd.tokenizer import ByteTokenizer
    mark("imports")

    cfg = {"llama3-8b": C.LLAMA3_8B, "llama3-70b": C.LLAMA3_70B, "llama32-1b": C.LLAMA32_1B,
           "qwen3-30b-a3b": C.QWEN3_30B_A3B, "qwen3-8b": C.QWEN3_8B}[args.model]
    if dev.type == "cpu":  # plumbing only (row-parallel shards need whole 256-wide super-blocks)
        if args.tp > 2:  # 8-way row-parallel shards (config #3's layout: 1 KV head per rank at tp 8)
            cfg = C.tiny_config(hidden=2048, ffn=4096, n_heads=16, n_kv_heads=8, head_dim=128, rope_dim=128)
        else:
            cfg = C.tiny_config(hidden=512, ffn=1024, n_heads=8, n_kv_heads=2)
    tp, link, tp_group, dp = args.tp, None, None, world
    tp_rel = None
    rehearsal = args.tp_rehearsal
    if rehearsal and (world > 1 or tp > 1):
        raise SystemExit("--tp-rehearsal runs one process (no --tp, no torchrun)")
    if tp > 1:
        link, tp_group, dist_leaders, dp = setup_tp(args, world, rank, dev)
        if not args.no_tp_check:
            # the measured sharded graph against the unsharded one: 2 layers of the same architecture,
            # identical weights, one prefill step (parallel/tp_engine.tp_selfcheck)
            import copy
            from localai_tfp_amd.parallel.tp_engine import tp_selfcheck
            small = copy.deepcopy(cfg)
            small.n_layers = 2
            tp_rel = tp_selfcheck(small, synthetic_source(small, "Q4_K_M", seed=3), dev, link.rank, tp, tp_group)
            if tp_rel is not None:
                print(f"[bench rank {rank}] tp self-check: max|dlogit|/max|logit| = {tp_rel:.2e}", file=sys.stderr,
                      flush=True)
        dist = dist_leaders  # bench barriers / reductions run among the replica leaders only
    t0 = time.time()
    src = synthetic_source(cfg, args.ftype, seed=1, shard_gen=tp > 1 or rehearsal > 1)
    if rehearsal > 1:
        model = LlamaModel.load(cfg, src, dev, 0, rehearsal, None)
    elif tp == 1:
        model = LlamaModel.load(cfg, generated_ahead(src), dev)
    else:
        model = LlamaModel.load(cfg, src, dev, rank % tp, tp, tp_group)
    t_load = time.time() - t0
    mark("load")
    if args.tokenizer == "bpe" and cfg.vocab != 128256:  # CPU plumbing model / other vocabularies
        args.tokenizer = "byte"
    tok = make_tokenizer(args.tokenizer, cfg.vocab)
    mark("tokenizer")
    ecfg = EngineConfig(max_num_seqs=args.concurrency, max_batched_tokens=args.max_batched_tokens,
                        prefill_chunk=args.prefill_chunk or None,
                        max_model_len=max(4096, args.prompt_len + args.gen_len + 64), use_graphs=not args.no_graphs,
                        kv_dtype=args.kv_dtype)
    if dev.type == "cpu":
        ecfg.num_blocks = 2048
    eng = LLMEngine(model, tok, ecfg, tp=link)
    mark("engine")
    if link is not None and not link.is_leader:
        eng.follow()  # replay the leader's plans until it stops the engine
        link.close()
        import torch.distributed as tdist
        tdist.destroy_process_group()
        return
    t0 = time.time()
    n_graphs = eng.precapture_graphs()
    t_capture = time.time() - t0
    mark("capture")

    if args.path == "http":
        res = run_http(args, eng, tok, cfg, dev, dist)
    else:
        res = run_engine(args, eng, tok, dev, dist)
    mark("serving")
    st = _host_snapshot(eng)  # the serving run's counters (the probe batch of --dump-outputs adds its own steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(args, eng, tok, args.phases.split(",")[0], args.dump_outputs)
        mark("dump")
    if args.path != "http":
        eng.shutdown()  # tensor parallel: releases the followers from engine.follow()
    t_el, tokens, ttfts, extra = res[0]
    bad_window = False
    phase_extra = {}
    for ph, (t2, tok2, tt2, ex2) in zip(args.phases.split(",")[1:], res[1:]):
        phase_extra[ph] = {"value": round(tok2 / t2, 2) if t2 else None,
                           "p50_ttft_ms": round(float(np.percentile(tt2, 50)), 2) if len(tt2) else None,
                           "p99_ttft_ms": round(float(np.percentile(tt2, 99)), 2) if len(tt2) else None,
                           "ms_per_step": round(t2 / args.steps * 1e3, 3), **{k: ex2[k] for k in (
                               "client_completed_requests", "ttft_samples", "p50_itl_ms", "window_engine_steps",
                               "window_prompt_tokens", "window_output_tokens") if k in ex2}}

    p50 = float(np.percentile(ttfts, 50)) if len(ttfts) else float("nan")
    p99 = float(np.percentile(ttfts, 99)) if len(ttfts) else float("nan")
    t_max, tok_sum, p50_all, p99_all = t_el, float(tokens), p50, p99
    if dist:
        single = args.path == "http" and args.dp_gateway == "single" and world > 1
        if single and rank != 0:
            p50 = p99 = 0.0  # the client-side latencies are rank 0's load generators'
        tt = torch.tensor([t_el, float(tokens), p50, p99], device=dev, dtype=torch.float64)
        mx = tt.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm = tt.clone()
        dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        t_max, tok_sum = float(mx[0]), float(sm[1])
        p50_all, p99_all = float(sm[2] / (1 if single else dp)), float(mx[3])
    value = tok_sum / t_max
    from localai_tfp_amd.ops.linear import ACT_DTYPE
    # 16-bit MFMA operands (Q4_K_M weights dequantised in-register), fp32 accumulation everywhere
    act_name = "fp16" if ACT_DTYPE == torch.float16 else "bf16"
    if rank == 0:
        out = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "output tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(t_max / args.steps * 1e3, 3),
            "step_unit": f"{args.step_group} engine iterations (continuous-batching forwards)",
            "ms_per_engine_iteration": round(t_max / (args.steps * args.step_group) * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": act_name,
            "data": f"synthetic (random-init {cfg.name} weights in real {args.ftype} block formats; synthetic chat prompts)",
            "p50_ttft_ms": round(p50_all, 2),
            "p99_ttft_ms": round(p99_all, 2),
            "config": {
                "model": cfg.name + " " + args.ftype, "global_batch": args.concurrency * dp,
                "seq_len": args.prompt_len + args.gen_len, "prompt_len": args.prompt_len, "gen_len": args.gen_len,
                "concurrency_per_replica": args.concurrency,
                "parallelism": (f"tp{rehearsal}-rehearsal (rank 0 shard on 1 GPU, collectives no-op)" if rehearsal > 1 else
                                f"dp{dp}" if tp == 1 else (f"tp{tp}" if dp == 1 else f"dp{dp}xtp{tp}")),
                **({"tp_selfcheck_rel_err": tp_rel} if tp_rel is not None else {}),
                "path": ("HTTP /v1/chat/completions (SSE) -> FastAPI gateway -> mxstream (batched gRPC-side channel) -> LLM worker engine" if args.path == "http"
                         else "engine in-process (gateway/gRPC excluded)"),
                **({"dp_gateway": args.dp_gateway if world > 1 else "single",
                    "gateway_workers": args.gateway_workers or (world if args.dp_gateway == "single" and world > 1 else 1)}
                   if args.path == "http" else {}),
                "load_s": round(t_load, 1), "gemm_tune_s": round(getattr(eng, "stats_tune_s", 0.0), 1),
                "graph_capture_s": round(t_capture, 1), "graphs": n_graphs, "timeline_s": TIMELINE,
                "graph_steps": st["graph_steps"], "total_steps": st["steps"],
                "host_ms_per_step": {k[:-2]: round(st[k] / max(1, st["steps"]) * 1e3, 3)
                                     for k in ("sched_s", "plan_s", "fwd_s", "wait_s", "process_s")},
                "graph_replay_host_ms": round(st["replay_s"] / max(1, st["graph_steps"]) * 1e3, 3),
                "weights_gb": round(model.weight_bytes() / 1e9, 2),
                "dense_weight_copy_gb": round(model.dense_cache_bytes() / 1e9, 2) if hasattr(model, "dense_cache_bytes") else 0.0, "kv_blocks": eng.kv.num_blocks,
                "kv_dtype": args.kv_dtype,
                "tokenizer": ("synthetic Llama-3-sized byte-level BPE (128,256 ids) through the GGUF BPE tokenizer"
                              if args.tokenizer == "bpe" else "byte"),
                "sampling": {"phase": args.phases.split(",")[0], **SAMPLING[args.phases.split(",")[0]]},
                **({"other_phases": phase_extra} if phase_extra else {}),
                "host_gc": {k: round(v, 4) for k, v in __import__("localai_tfp_amd.engine.engine",
                                                                  fromlist=["GC_STATS"]).GC_STATS.items()},
                **extra,
            },
        }
        print(json.dumps(out), flush=True)
        n_tt = extra.get("ttft_samples")
        if args.min_ttft_samples and n_tt is not None and n_tt < args.min_ttft_samples and not rehearsal:
            print(f"[bench] only {n_tt} TTFT samples fell in the timed window (< {args.min_ttft_samples}): the window "
                  "did not time a representative serving mix", file=sys.stderr, flush=True)
            bad_window = args.full  # a plain run reports the count and the warning; --full fails on it
        if eng.trace is not None:
            torch.cuda.synchronize() if dev.type == "cuda" else None
            ev = eng.trace_events[-(args.steps * args.step_group + 50):]
            # device time of each step (launch marker -> sampler end) and the device idle before the next one
            gpu = [[a.elapsed_time(b), b.elapsed_time(c)] for (a, b), (c, _) in zip(ev, ev[1:])]
            with open(os.environ["MX_STEP_TRACE"], "w") as f:
                json.dump({"host": eng.trace, "gpu_ms": gpu}, f)
        if os.environ.get("MX_TUNE_REPORT"):
            from localai_tfp_amd.ops import autotune
            with open(os.environ["MX_TUNE_REPORT"], "w") as f:
                json.dump(autotune.report(), f, indent=1)
    if link is not None:
        link.close()
    if world > 1:
        import torch.distributed as tdist
        tdist.destroy_process_group()
    mark("exit")
    if rank == 0:
        print(f"[bench] timeline_s {TIMELINE}", file=sys.stderr, flush=True)
    if bad_window:
        sys.exit(3)


class Window:
    """Engine-thread hook that times exactly K engine steps of the STEADY serving state.

    Steady state: at least `steady_finished` requests have completed since the load started (with
    the load generator's staggered first lengths, completions and re-arrivals are then spread
    evenly, so every step holds the stationary mix of decode rows plus arriving prefill chunks).
    From the first steady step, W more steps run untimed (the driver's warmup), then sync +
    barrier, t0, K steps, sync + barrier, t1. Under DP every rank gates on its own engine and
    the barrier aligns the windows.
    """

    def __init__(self, eng, warmup, steps, dev, dist, steady_finished: int, base_finished: int = 0):
        # warmup / steps are ENGINE ITERATIONS here (the caller multiplies bench steps by the step group)
        self.eng, self.W, self.K, self.dev, self.dist = eng, warmup, steps, dev, dist
        self.pre0 = self.pre1 = 0
        self.steady_finished = steady_finished + base_finished
        self.steady_step = None
        self.t0 = self.t1 = None
        self.tok0 = self.tok1 = 0
        self.done = threading.Event()

    def _sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        if self.dist:
            self.dist.barrier()

    def __call__(self, i):
        if self.steady_step is None:
            if self.eng.stats["finished"] < self.steady_finished:
                return
            self.steady_step = i
        j = i - self.steady_step
        if j == self.W and self.t0 is None:
            self._sync()
            self.t0 = time.monotonic()
            self.tok0 = self.eng.stats["out_tokens"]
            self.pre0 = self.eng.stats["prefill_tokens"]
            self.step0 = i
        elif j == self.W + self.K and self.t1 is None:
            self._sync()
            self.t1 = time.monotonic()
            self.tok1 = self.eng.stats["out_tokens"]
            self.pre1 = self.eng.stats["prefill_tokens"]
            self.done.set()


def steady_gate(args) -> int:
    """Completed requests after which the serving mix is stationary (see Window)."""
    # two full generations of the concurrency: every request that was running at the load's start has been replaced
    # and the replacements' ages are spread evenly, so a small driver W no longer times the ramp (with the round-4
    # gate of half a generation, the phase after a first one ran 2-3 % faster than that first phase on the same box;
    # with W = 800 the two agreed — profiles/r5_step_composition.md)
    return args.steady_finished if args.steady_finished >= 0 else max(1, 2 * args.concurrency)


def run_http(args, eng, tok, cfg, dev, dist):
    """One gateway + worker; one closed-loop load generator per sampling phase, each with its own
    steady-state window. Returns [(window_s, tokens, ttfts, extra)] per phase."""
    import yaml
    from localai_tfp_amd.grpc.server import AioServer
    from localai_tfp_amd.workers.llm import LLMServicer

    sys.setswitchinterval(0.0005)  # same as workers/llm.py main(): engine thread + gRPC loop share the GIL
    svc = LLMServicer(device=str(dev))
    svc.attach(eng, tok)
    eng.start()
    server = AioServer(svc, "127.0.0.1:0", max_workers=16)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    single = args.dp_gateway == "single" and dist is not None and world > 1
    front = not single or int(os.environ.get("RANK", "0")) == 0
    if single:
        # every rank's worker address to rank 0, whose one gateway fronts them all as data-parallel replicas
        pt = torch.zeros(world, dtype=torch.int64, device=dev)
        pt[int(os.environ.get("RANK", "0"))] = server.port
        dist.all_reduce(pt)
        backends = "|".join(f"127.0.0.1:{int(p)}" for p in pt.tolist())
        conc, n_gw = args.concurrency * world, args.gateway_workers or world
    else:
        backends, conc, n_gw = f"127.0.0.1:{server.port}", args.concurrency, args.gateway_workers or 1
    work = tempfile.mkdtemp(prefix="mxbench")
    models = os.path.join(work, "models")
    os.makedirs(models)
    with open(os.path.join(models, "llama-3-8b-instruct.yaml"), "w") as f:
        yaml.safe_dump({"name": "llama-3-8b-instruct", "backend": "llama-cpp",
                        "context_size": eng.cfg.max_model_len,
                        "parameters": {"model": f"synthetic:{args.model}"},
                        "template": {"use_tokenizer_template": True},
                        "known_usecases": ["chat"]}, f)
    port = free_port()
    env = dict(os.environ)
    env["LOCALAI_GPUS"] = "none"          # the gateway never touches the GPU
    env.pop("RANK", None), env.pop("WORLD_SIZE", None), env.pop("LOCAL_RANK", None)
    gw_log = open(os.path.join(work, "gateway.log"), "w")
    gw = subprocess.Popen([sys.executable, "-m", "localai_tfp_amd", "run", "--models-path", models,
                           "--address", f"127.0.0.1:{port}", "--disable-webui", "--log-level", "warning",
                           "--localai-config-dir", os.path.join(work, "cfg"),
                           "--generated-content-path", os.path.join(work, "gen"),
                           "--upload-path", os.path.join(work, "up"), "--gateway-workers", str(n_gw),
                           "--external-grpc-backends", f"llama-cpp:{backends}"],
                          env=env, cwd=ROOT, stdout=gw_log, stderr=subprocess.STDOUT,
                          start_new_session=True) if front else None
    if args.tokenizer == "byte":
        size_args = ["--prompt-chars", str(max(1, args.prompt_len - TEMPLATE_OVERHEAD))]
    else:
        _, n_words = prompt_sizing(tok, args.prompt_len)
        size_args = ["--prompt-words", str(n_words)]
    out = []
    n_lg = max(1, min(world, 4)) if single else 1  # one asyncio load generator carries ~25k chunks/s
    try:
        if front:
            wait_http(f"http://127.0.0.1:{port}/readyz", 120, gw)
        mark("gateway")
        for pi, phase in enumerate(args.phases.split(",")):
            sp = SAMPLING[phase]
            samp_args = ["--temperature", str(sp["temperature"])]
            if "top_k" in sp:
                samp_args += ["--top-k", str(sp["top_k"]), "--top-p", str(sp["top_p"])]
            if sp.get("frequency_penalty"):
                samp_args += ["--frequency-penalty", str(sp["frequency_penalty"])]
            if sp.get("json"):
                samp_args += ["--json"]
            win = Window(eng, args.warmup * args.step_group, args.steps * args.step_group, dev, dist, steady_gate(args),
                         base_finished=eng.stats["finished"])
            eng.on_step = win
            rec_paths = [os.path.join(work, f"loadgen_{pi}_{i}.json") for i in range(n_lg)] if front else []
            lgs = [subprocess.Popen([sys.executable, "-m", "localai_tfp_amd.tools.loadgen",
                                     "--url", f"http://127.0.0.1:{port}", "--model", "llama-3-8b-instruct",
                                     "--concurrency", str(conc // n_lg + (i < conc % n_lg)), *size_args, *samp_args,
                                     "--gen-len", str(args.gen_len),
                                     "--seed", str(int(os.environ.get("RANK", "0")) + 97 * pi + 1000 * i),
                                     "--stagger", "--out", rp], env=env, cwd=ROOT, start_new_session=True)
                   for i, rp in enumerate(rec_paths)]
            try:
                t_start = time.time()
                last = -1
                while not win.done.wait(30):
                    n = eng.stats["steps"]
                    print(f"[bench rank {os.environ.get('RANK', '0')}] phase={phase} steps={n} "
                          f"out_tokens={eng.stats['out_tokens']}", file=sys.stderr, flush=True)
                    if any(lg.poll() is not None for lg in lgs) or (gw is not None and gw.poll() is not None):
                        raise RuntimeError("load generator or gateway exited early; see " + work)
                    if time.time() - t_start > args.timeout or (n == last and n > 0):
                        raise TimeoutError(f"window not reached (steps={n}); see {work}")
                    last = n
            finally:
                eng.on_step = None
                for lg in lgs:
                    if lg.poll() is None:
                        lg.send_signal(signal.SIGTERM)
                for lg in lgs:
                    try:
                        lg.wait(timeout=60)
                    except subprocess.TimeoutExpired:
                        lg.kill()
            out.append(_http_phase_result(win, rec_paths))
            mark(f"window_{phase}")
            # the cancelled streams of this phase must leave the engine before the next phase's gate counts
            t_d = time.time()
            while (eng.sched.running or eng.sched.waiting) and time.time() - t_d < 120:
                time.sleep(0.1)
    finally:
        eng.on_step = None
        if single:  # the gateway (rank 0) still holds connections to every rank's worker
            dist.barrier()
        eng.shutdown()
        if gw is not None:
            gw.terminate()
            try:
                gw.wait(timeout=20)
            except subprocess.TimeoutExpired:
                gw.kill()
        server.stop()
    return out


def _http_phase_result(win, rec_paths):
    recs = []
    for rp in rec_paths:
        try:
            with open(rp) as f:
                recs += json.load(f)
        except (OSError, ValueError):
            pass
    t0, t1 = win.t0, win.t1
    ttfts = [(r["t_first"] - r["t_send"]) * 1e3 for r in recs if r.get("t_first") and t0 <= r["t_first"] <= t1]
    done = [r for r in recs if r.get("ok") and t0 <= r["t_end"] <= t1]
    client_tps = sum(r["tokens"] for r in done) / (t1 - t0) if done else 0.0
    errors = sum(1 for r in recs if r.get("error") not in (None, "CancelledError"))
    window = {"window_engine_steps": win.K, "window_prompt_tokens": win.pre1 - win.pre0,
              "window_output_tokens": win.tok1 - win.tok0}
    if not recs:  # a rank behind the single DP gateway: its engine's tokens count, the client side is rank 0's
        return t1 - t0, win.tok1 - win.tok0, [], {"steady_at_step": win.steady_step, **window}
    # inter-token latency: gaps between consecutive content chunks of one stream, both inside the window
    itl = [(b - a) * 1e3 for r in recs for a, b in zip(r.get("t_chunks", []), r.get("t_chunks", [])[1:])
           if t0 <= a and b <= t1]
    chunks_in = sum(1 for r in recs for t in r.get("t_chunks", []) if t0 <= t <= t1)
    extra = {"client_completed_requests": len(done), "client_tokens_per_s_completed": round(client_tps, 1),
             "client_chunks_per_s": round(chunks_in / (t1 - t0), 1),
             "http_errors": errors, "ttft_samples": len(ttfts),
             "p50_itl_ms": round(float(np.percentile(itl, 50)), 2) if itl else None,
             "p99_itl_ms": round(float(np.percentile(itl, 99)), 2) if itl else None,
             "steady_at_step": win.steady_step, "window_first_step": getattr(win, "step0", None), **window}
    return t1 - t0, win.tok1 - win.tok0, ttfts, extra


def run_engine(args, eng, tok, dev, dist):
    from localai_tfp_amd.engine.sequence import Request
    from localai_tfp_amd.ops.sampling import SamplingParams
    make_prompt = prompt_maker(args, tok, np.random.default_rng(1234 + int(os.environ.get("RANK", "0"))))
    phase = args.phases.split(",")[0]
    if SAMPLING[phase].get("json"):
        raise SystemExit("the json phase needs the HTTP path (response_format is an API-level option)")
    sp = SamplingParams(**SAMPLING[phase], ignore_eos=True) if phase != "greedy" else \
        SamplingParams(temperature=0.0, top_k=1, ignore_eos=True)
    handles = {}
    ttfts = []
    timed = {"on": False}

    def submit(gen=None):
        req = Request(make_prompt(), sp, max_tokens=gen or args.gen_len)
        handles[req.rid] = (eng.submit(req), time.monotonic())

    C = args.concurrency
    for i in range(C):  # staggered first lengths (see tools/loadgen.py --stagger)
        submit(-(-args.gen_len * (i + 1) // C))

    def drain():
        done = []
        for rid, (h, t_sub) in list(handles.items()):
            while not h.q.empty():
                o = h.q.get_nowait()
                if o.token_ids and not getattr(h, "_first", False):
                    h._first = True
                    if timed["on"]:
                        ttfts.append((time.monotonic() - t_sub) * 1e3)
                if o.finished:
                    done.append(rid)
        for rid in done:
            handles.pop(rid)
            submit()

    def step():
        eng._drain_inbox()
        eng.step()
        drain()

    gate = steady_gate(args)
    n_pre = 0
    while eng.stats["finished"] < gate and n_pre < 100000:
        step()
        n_pre += 1
    G = args.step_group
    for _ in range(args.warmup * G):
        step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    if dist:
        dist.barrier()
    timed["on"] = True
    tok0 = eng.stats["out_tokens"]
    pre0 = eng.stats["prefill_tokens"]
    s0 = _host_snapshot(eng)
    t_start = time.monotonic()
    for _ in range(args.steps * G):
        step()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    if dist:
        dist.barrier()
    t_el = time.monotonic() - t_start
    return [(t_el, eng.stats["out_tokens"] - tok0, ttfts, {
        "steady_at_step": n_pre, "window_host": _host_delta(s0, _host_snapshot(eng)), "ttft_samples": len(ttfts),
        "window_engine_steps": args.steps * G, "window_prompt_tokens": eng.stats["prefill_tokens"] - pre0,
        "window_output_tokens": eng.stats["out_tokens"] - tok0})]


def _host_snapshot(eng):
    st = dict(eng.stats)
    st["replay_s"] = sum(g.replay_s for g in eng.graphs.values())
    return st


def _host_delta(a, b):
    """Host-side engine time per step inside the timed window (ms): scheduler, plan, launch (fwd),
    wait for the in-flight step, post-processing; plus how many window steps replayed a hipGraph."""
    n = max(1, b["steps"] - a["steps"])
    out = {k[:-2] + "_ms": round((b[k] - a[k]) / n * 1e3, 3)
           for k in ("sched_s", "plan_s", "fwd_s", "wait_s", "process_s", "replay_s")}
    out["steps"] = b["steps"] - a["steps"]
    out["graph_steps"] = g = b["graph_steps"] - a["graph_steps"]
    out["fwd_graph_step_ms"] = round((b["fwd_graph_s"] - a["fwd_graph_s"]) / max(1, g) * 1e3, 3)
    out["fwd_eager_step_ms"] = round((b["fwd_s"] - a["fwd_s"] - b["fwd_graph_s"] + a["fwd_graph_s"]) / max(1, n - g) * 1e3, 3)
    out["prefill_tokens_per_step"] = round((b["prefill_tokens"] - a["prefill_tokens"]) / n, 1)
    return out


if __name__ == "__main__":
    main()
