#!/usr/bin/env python
"""bench.py — headline benchmark of the EdgeCape hot path on MI355X (contract: see the task prompt §④).

A "step" is one pass of the device-side `forward_test` (DINOv2 backbone on query + support images, then
the support<->query keypoint head) over one batch of synthetic (support, query) pairs that are already
resident in HBM.  Workload at any N: BASELINE.json configs[1] per GPU — 1-shot, 32 pairs of 256x256,
DINOv2 ViT-B/14 (18x18 token grid, floor semantics) — i.e. weak scaling: rank r processes its own shard
of pairs (seeded by the global pair index), no data-path collective; one RCCL all-reduce of the PCK
counters at the end.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps, writes the last step's outputs if `--dump-outputs DIR` is given, and prints the
headline line.  Every other leg (PCK and conformance records, `sustained`, the episode protocol, the CPU baseline and parity sample,
the unpipelined / conforming / bf16 comparison runs) runs only with `--full`; the `--no-*` switches choose among them there.

Prints ONE JSON line on rank 0.  `roofline` is for the north-star kernel (backbone QKV GEMM, its own
kernel symbol gemm8_bf16_kernel<1, 1, ..>): algorithmic FLOPs per launch / mean launch duration measured with
HIP events bracketing one launch per timed step, the block rotating with the step (ec_profile mode 2).  `cpu_baseline` times the CPU
oracle (a port, not the product) on the host cores over a bounded sample of the same workload.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# /opt/skills/guides/MI355X_MICROARCH.md: dense MFMA peaks (2500 TFLOP/s 16-bit, 5000 FP8).  bf16x3: three 16-bit MFMAs per product; fp16x2: one
# fp16 MFMA + a depth-2K FP8 pass at twice the rate = two 16-bit-MFMA units per product
PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "bf16x3": 2500.0 / 3, "fp16x2": 2500.0 / 2, "fp32": 157.3}


CONFORMING = ("fp16x2", "bf16x3")   # backbone / head precision of the tolerance-conforming mode the default line reports beside the headline


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24,
                    help="timed steps (default 24 = two passes over the 12 backbone blocks: the QKV launch sampled in step i is block i %% depth, "
                         "so every block weighs the same in roofline.frac - the early blocks of a pipelined step share the chip with the "
                         "previous step's head, the late ones do not)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="pairs per GPU per step (configs[1]: 32)")
    ap.add_argument("--shots", type=int, default=1)
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--arch", default="dinov2_vitb14")
    ap.add_argument("--precision", default=os.environ.get("EC_BENCH_PRECISION", "fp16"), choices=["bf16", "fp16", "bf16x3", "fp16x2", "fp32"],
                    help="backbone MFMA operand type (fp32 accumulate).  Default fp16: same MFMA rate as bf16, 8x smaller rounding - the "
                         "fastest mode whose keypoints stay inside the 1e-3 tolerance (tests/test_gpu_precision_modes.py)")
    ap.add_argument("--head-precision", default=os.environ.get("EC_BENCH_HEAD_PRECISION", "mixed"), choices=["fp32", "bf16x3", "mixed"],
                    help="head GEMMs: exact fp32 MFMA, or split-bf16 (hi+lo, 3 MFMAs per product; fp32-class accuracy)")
    ap.add_argument("--cpu-batches", default="2,32", help="batch sizes of the CPU-baseline protocol (BASELINE.md §4)")
    ap.add_argument("--cpu-runs", type=int, default=5, help="timed CPU forwards per batch size (after 2 warm-ups)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-episode", action="store_true", help="skip the episode-protocol measurement (ec_forward_episodes)")
    ap.add_argument("--episode-images", type=int, default=0,
                    help="backbone images per call of the episode leg (queries + support images of the episodes that start in it); "
                         "0 = as many as a headline step, (1 + shots) * batch")
    ap.add_argument("--sustained-seconds", type=float, default=5.0,
                    help="length of the `sustained` leg: pipelined steps for about this long in the same process (0: skip).  `value` stays the "
                         "K timed steps of the contract - a 0.1 s burst; this leg says what the path holds once the clock has settled")
    ap.add_argument("--no-alt", action="store_true", help="skip the short bf16 / unpipelined comparison runs")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="time ec_forward (every call complete at its own end) instead of ec_forward_pipelined (the decoder phase of "
                         "step i runs beside the backbone of step i+1; all work of the K steps still lies inside the timed region)")
    ap.add_argument("--full", action="store_true",
                    help="run every leg beside the headline as well: PCK vs the synthetic ground truth, the conformance records, "
                         "`sustained`, the episode protocol, the CPU baseline + parity sample and the comparison runs (the --no-* "
                         "switches above choose among them).  Off: only the headline's warm-up and K timed steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step (rank 0's shard; what forward_test's device "
                         "part hands its caller) as DIR/<name>.npy in float32, at most 64 MB in all (a fixed, seeded sample of the "
                         "pairs beyond that)")
    return ap.parse_args()


def main():
    args = parse()
    import torch
    from edgecape_amd import synth
    from edgecape_amd.engine import HipEngine
    from edgecape_amd.evaluation import pck_counts, pck_from_counts
    from edgecape_amd import apis, _lib, build

    # one process per GPU; the same helpers the world-size-2 gloo tests drive (tests/test_dist_gloo.py)
    # backend: RCCL ("nccl") whenever a GPU is visible; gloo only without one (tests/test_dist_gloo.py drives this function with
    # world size 2 and a stand-in engine on CPU so that the N > 1 branches below run before an 8-GPU job does)
    rank, world, local_rank = apis.init_distributed(None)
    device = "cuda" if torch.cuda.is_available() else "cpu"
    if world != args.gpus and rank == 0:
        print(f"[bench] warning: --gpus {args.gpus} but WORLD_SIZE {world}", file=sys.stderr)

    bs, S, H, arch = args.batch, args.shots, args.image_size, args.arch
    a = synth.ARCHS[arch]
    C, depth = a["C"], a["depth"]
    g = H // 14
    T = g * g + 1
    sd = synth.make_weights(arch, seed=0)

    # this rank's shard: global pair indices rank*bs .. rank*bs+bs-1 (fixed per-GPU work => weak scaling)
    batch = synth.make_pairs(bs, S, H, seed=1000, first_index=rank * bs, fixed_n_kp=False)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)   # (no GPU: HipEngine below refuses - there is no CPU path)
    iq = dev(batch["img_q"])
    is_ = [dev(x) for x in batch["img_s"]]
    ts = [dev(x) for x in batch["target_s"]]
    mask = batch["target_weight_s"][0].copy()
    for tw in batch["target_weight_s"]:
        mask = mask * tw
    ms = dev(mask.reshape(bs, -1))

    def timed_run(precision, steps, warmup, profile, pipelined=True, head_precision=None, eng=None):
        """`warmup` + `steps` passes of the hot path in `precision`; returns (engine, outputs, seconds (max over ranks), mean QKV launch ms).
        pipelined: ec_forward_pipelined with two alternating output sets - step i's decoder phase runs beside step i+1's backbone -
        and an ec_pipeline_flush inside the timed region, so that all the work of the K steps is charged to them."""
        if eng is None:
            eng = HipEngine(sd, arch=arch, image_size=H, max_batch=bs, max_shots=S, backbone_precision=precision,
                            head_precision=head_precision or args.head_precision)
        edges, off = eng._edges([m["sample_skeleton"][0] for m in batch["img_metas"]], bs)
        sets = [eng._outputs(bs), eng._outputs(bs)]
        count = [0]

        def step():
            outs = sets[count[0] & 1]
            count[0] += 1
            if pipelined:
                eng.forward_pipelined(iq, is_, ts, ms, edges, off, outs)
            else:
                eng.forward_resident(iq, is_, ts, ms, edges, off, outs)

        def closing():
            if pipelined:
                eng.pipeline_flush()           # the last step's decoder: inside the timed region
            # the only cross-GPU exchange of the job: the PCK counters (their values are computed after the timed region from the
            # last step's outputs; the collective itself sits inside the timed region so its cost is charged)
            apis.allreduce_counts(np.zeros(6))

        # sampled (mode 2): ONE QKV launch per step is bracketed by HIP events, the block rotating with the step - an event pair costs
        # the stream two ~6 us barrier packets, and bracketing all 12 launches of a step put 2 % of idle time into the timed region
        arm = (lambda: _lib.check(eng.lib.ec_profile(eng.h, 2, steps))) if profile else None
        dt = apis.timed_steps(step, steps, warmup, collective=closing, before_timed=arm)
        outputs = sets[(count[0] - 1) & 1]
        qkv_ms = 0.0
        if profile:
            import ctypes as Ct
            tot_ms, nl = Ct.c_float(), Ct.c_int()
            _lib.check(eng.lib.ec_profile_read(eng.h, Ct.byref(tot_ms), Ct.byref(nl)))
            _lib.check(eng.lib.ec_profile(eng.h, 0, 0))
            qkv_ms = tot_ms.value / max(nl.value, 1)
        timed_run.launches = nl.value if profile else 0
        return eng, outputs, dt, qkv_ms

    pipelined = not args.no_pipeline
    eng, outputs, dt, qkv_ms = timed_run(args.precision, args.steps, args.warmup, True, pipelined)
    launches_timed = timed_run.launches
    Mq, Kq, Nq = (1 + S) * bs * T, C, 3 * C
    qkv_flops = 2.0 * Mq * Kq * Nq
    achieved = qkv_flops / (qkv_ms * 1e-3) / 1e12 if qkv_ms > 0 else 0.0
    peak = PEAK_TFLOPS[args.precision]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, outputs[0])

    pck = None
    if args.full:
        # ---- accuracy bookkeeping on this rank's last outputs: PCK vs the synthetic ground truth (random weights: chance level; the
        # meaningful agreement figures are in `parity_sample`: HIP predictions against the oracle's on the same pairs)
        out_k = outputs[0]["output_kpts"][-1].cpu().numpy()            # [bs,K,2] normalised
        scale200 = np.stack([m["query_scale"] for m in batch["img_metas"]]) * 200.0
        center = np.stack([m["query_center"] for m in batch["img_metas"]])
        pred_px = out_k * H * (scale200 / H)[:, None, :] + center[:, None, :] - scale200[:, None, :] * 0.5
        vis = (mask[:, :, 0] > 0) & (batch["target_weight_q"][:, :, 0] > 0)
        norm = np.full((bs, 2), float(H))
        counts = pck_counts(pred_px, batch["gt_q"], vis, norm)
        counts = apis.allreduce_counts(counts)
        pck = pck_from_counts(counts)

    # ---- legs that run on EVERY rank (their timed regions carry the same barriers / max over ranks as the headline's)
    sustained = None
    if args.full and args.sustained_seconds > 0 and pipelined:
        n_s = max(args.steps, int(np.ceil(args.sustained_seconds / (dt / args.steps))))
        _, _, dt_s, qkv_s = timed_run(args.precision, n_s, 0, True, True, eng=eng)
        ach_s = qkv_flops / (qkv_s * 1e-3) / 1e12 if qkv_s > 0 else 0.0
        sustained = {"value": round(world * bs * n_s / dt_s, 2), "unit": "images/s", "steps": n_s, "seconds": round(dt_s, 6),
                     "ms_per_step": round(dt_s / n_s * 1e3, 3), "qkv_frac": round(ach_s / peak, 4), "qkv_launch_ms": round(qkv_s, 5),
                     "launches_timed": timed_run.launches,
                     "note": "the same pipelined steps for >= %.0f s in the same process, same engine, right after the K timed steps of `value`" % args.sustained_seconds}
    episode = None
    if args.full and not args.no_episode:
        episode = episode_mode(args, sd, synth, bs, S, H, arch, apis, rank, world, parity_episodes=0 if args.no_cpu_baseline else 2)
        if not args.episode_images and torch.cuda.is_available():
            # the same protocol in calls of twice the size (288 GB of HBM: the call size is free; the head's ~190 launches per call
            # are then shared by twice the queries)
            big = episode_mode(args, sd, synth, bs, S, H, arch, apis, rank, world, n_img=2 * (1 + S) * bs)
            episode["calls_of_twice_the_size"] = {k: big[k] for k in ("value", "queries_per_call", "calls_per_pass", "ms_per_call", "seconds")}

    result = None
    if rank == 0:
        value = world * bs * args.steps / dt
        dname = {"bf16": "bf16", "fp16": "f16", "bf16x3": "bf16x3", "fp16x2": "f16+fp8", "fp32": "f32"}
        result = {
            "metric": "query images/sec (1-shot, 256x256, DINOv2 ViT-B/14 + EdgeCape head, forward_test)",
            "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dname[args.precision], "data": "synthetic",
            "pipelined": pipelined,   # ec_forward_pipelined: step i's decoder phase beside step i+1's backbone (`unpipelined`: ec_forward)
            "config": {"workload": f"{S}-shot split1-style synthetic pairs, batch={bs}/GPU, {H}x{H}, {arch}, K=100 padded keypoints, "
                                   f"backbone {args.precision} MFMA / fp32 accumulate, head {args.head_precision}",
                       "global_batch": world * bs, "parallelism": f"dp{world} (independent pair shards, one all-reduce of PCK counters)"},
            "roofline": {"bound": "mfma", "kernel": f"backbone QKV GEMM M={Mq} K={Kq} N={Nq} ({args.precision})",
                         "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                         "flops_per_launch": qkv_flops, "avg_launch_ms": round(qkv_ms, 5), "launches_timed": launches_timed,
                         # achieved / frac / avg_launch_ms belong to the timed region that produced `value` (this run's K steps)
                         "measured_in": ("the timed region of `value`: the K ec_forward_pipelined steps - the sampled launches share the chip with "
                                         "the previous step's head" if pipelined else "the timed region of `value`: the K ec_forward steps - nothing else on the chip"),
                         "launch_sampling": "one QKV launch per step bracketed by HIP events on the launch stream, block index = step % depth",
                         **pmc_traffic(args, bs, S, H, arch, build.source_hash())},
            # every switch that changes what the library runs (README "Runtime switches"): none set = the shipped defaults
            "env": {k: v for k, v in sorted(os.environ.items()) if k.startswith("EC_")},
            "library_source_hash": build.source_hash()[:16],
        }
        if pck is not None:
            result["pck_vs_synthetic_gt"] = {k: round(v, 4) for k, v in pck.items()}
        conf = conformance_record(args, bs, S, H, arch) if args.full else None
        if conf:
            result["conformance_at_scale"] = conf
        if sustained:
            result["sustained"] = sustained
        if episode:
            result["episode_cached"] = episode
            result["episode_cached"]["speedup_vs_value"] = round(episode["value"] / result["value"], 3)
        if args.full and not args.no_cpu_baseline and world == 1:
            result["cpu_baseline"], result["parity_sample"] = cpu_baseline(args, sd, eng, synth)
    if args.full and world == 1 and not args.no_alt and pipelined:
        # the same steps through ec_forward (every call complete when the stream reaches its end), measured beside the headline
        del eng, outputs
        torch.cuda.empty_cache()
        n_u = max(5, args.steps // 2)
        eng, outputs, dt_u, qkv_u = timed_run(args.precision, n_u, args.warmup, True, False)
        result["unpipelined"] = {"value": round(bs * n_u / dt_u, 2), "unit": "images/s", "ms_per_step": round(dt_u / n_u * 1e3, 3),
                                 "qkv_launch_ms": round(qkv_u, 5), "qkv_frac": round(qkv_flops / (qkv_u * 1e-3) / 1e12 / peak, 4) if qkv_u > 0 else None,
                                 "note": "ec_forward: no overlap between steps; the QKV launches are not disturbed by a concurrent head"}
        # the reference's contract (forward_test returns complete results): the same steps through ec_forward
        result["value_reference_contract"] = result["unpipelined"]["value"]
        if qkv_u > 0:
            # The same kernel with the chip to itself (a second timed region of the same process through ec_forward, HIP events on the launch
            # stream as above; rocprofv3's kernel trace serialises kernels and agrees with THIS duration): a property of the KERNEL, kept
            # beside - not instead of - the figure of the timed region that produced `value`.
            ach_u = qkv_flops / (qkv_u * 1e-3) / 1e12
            result["roofline"]["kernel_isolated"] = {
                "achieved": round(ach_u, 2), "frac": round(ach_u / peak, 4), "avg_launch_ms": round(qkv_u, 5), "launches_timed": timed_run.launches,
                "measured_in": f"{n_u} timed ec_forward steps of this process (nothing else on the chip), one sampled launch per step"}
    if args.full and world == 1 and not args.no_alt and (args.precision, args.head_precision) != CONFORMING:
        # the tolerance-conforming fast mode, same process, same box, same API as the headline.  Round 6: fp16x2 backbone (a_hi W_hi in fp16
        # MFMAs + both correction terms in ONE block-scaled FP8 pass: two MFMA units per product instead of the three of bf16x3) + bf16x3
        # head; meets the 1e-3 coordinate tolerance on every keypoint but the near-ties any GPU summation order flips (0 / 2 / 1 / 1 argmax
        # flips of ~20 000 on cfg1 / 2 / 4 / 5 at scale, max 1.4e-5 elsewhere; tests/test_gpu_precision_modes.py::test_parity_mode_fp16x2)
        del eng, outputs
        torch.cuda.empty_cache()
        n_c = max(5, args.steps // 2)
        cb, ch = CONFORMING
        eng, outputs, dt_c, qkv_c = timed_run(cb, n_c, args.warmup, True, pipelined, head_precision=ch)
        ach_c = qkv_flops / (qkv_c * 1e-3) / 1e12 if qkv_c > 0 else 0.0
        conf_c = conformance_record(args, bs, S, H, arch, cb, ch)
        result["conforming_mode"] = {
            "precision": f"{cb} backbone / {ch} head", "value": round(bs * n_c / dt_c, 2), "unit": "images/s", "ms_per_step": round(dt_c / n_c * 1e3, 3),
            "pipelined": pipelined,
            "roofline": {"bound": "mfma", "achieved": round(ach_c, 2), "peak": round(PEAK_TFLOPS[cb], 1), "unit": "TFLOP/s",
                         "frac": round(ach_c / PEAK_TFLOPS[cb], 4), "avg_launch_ms": round(qkv_c, 5), "launches_timed": timed_run.launches,
                         "peak_note": "2500 / 2: two 16-bit-MFMA units per product (one fp16 MFMA + a depth-2K FP8 pass at twice the rate); "
                                      "`achieved` counts the layer's 2 M N K flops once"},
            "argmax_flips": conf_c.get("argmax_flips") if conf_c else None, "conformance_at_scale": conf_c,
            "note": "meets the 1e-3 coordinate tolerance on every keypoint but the measured near-tie flips; the headline precision meets it on all but its (larger) measured flip rate"}
        if not args.no_episode:
            # the reference's evaluation protocol (15 queries per support set, `episode_cached` above) in the conforming precision
            del eng, outputs
            torch.cuda.empty_cache()
            eng = outputs = None
            ep_c = episode_mode(args, sd, synth, bs, S, H, arch, apis, rank, world, precision=cb, head_precision=ch)
            result["conforming_mode"]["episode_cached"] = {k: ep_c[k] for k in ("value", "unit", "queries_per_call", "calls_per_pass", "ms_per_call", "seconds",
                                                                                 "backbone_images_per_pair", "entry_point")}
        # the round-5 conforming mode (three bf16 MFMAs per product) beside it, same process
        del eng, outputs
        torch.cuda.empty_cache()
        eng, outputs, dt_3, qkv_3 = timed_run("bf16x3", n_c, args.warmup, True, pipelined, head_precision="bf16x3")
        result["conforming_mode"]["bf16x3_bf16x3"] = {"value": round(bs * n_c / dt_3, 2), "unit": "images/s", "ms_per_step": round(dt_3 / n_c * 1e3, 3),
                                                      "qkv_launch_ms": round(qkv_3, 5), "note": "round 5's conforming mode: every product as three bf16 MFMAs"}
    if args.full and world == 1 and not args.no_alt and args.precision != "bf16":
        # the same step with bf16 operands (north_star's wording): same kernels and rate, 8x coarser rounding - measured beside the
        # headline so both precisions come from one process on one box; it does NOT meet the 1e-3 gate (test_bf16_mode_cfg2_bounded)
        del eng, outputs
        torch.cuda.empty_cache()
        _, _, dt_b, qkv_b = timed_run("bf16", max(5, args.steps // 2), args.warmup, True, pipelined)
        n_b = max(5, args.steps // 2)
        result["bf16_mode"] = {"value": round(bs * n_b / dt_b, 2), "unit": "images/s", "ms_per_step": round(dt_b / n_b * 1e3, 3),
                               "qkv_launch_ms": round(qkv_b, 5), "qkv_frac": round(qkv_flops / (qkv_b * 1e-3) / 1e12 / PEAK_TFLOPS["bf16"], 4) if qkv_b > 0 else None,
                               "note": "bf16 backbone operands; outside the 1e-3 tolerance (max 2.2e-3 on flip-free samples, 0.5 % argmax flips)"}
    if rank == 0:
        print(json.dumps(result), flush=True)
    apis.finalize_distributed()
    return result


DUMP_BYTES = 60 << 20                                    # array data --dump-outputs writes at most (64 MB with the .npy headers)
DUMP_PAIR_AXIS = {"output_kpts": 1, "attn_adj": 1, "out_points": 1}   # the others (engine._outputs) lead with the pair axis


def dump_outputs(path, outs, seed=0):
    """--dump-outputs: every output array of the last timed step as <path>/<name>.npy, float32.  When they exceed DUMP_BYTES together,
    one fixed, seeded sample of pairs (sorted, drawn from `seed` alone) is kept in every array, so that two builds dump the same entries."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    arrs = {k: v.detach().float().cpu().numpy() for k, v in outs.items() if isinstance(v, torch.Tensor)}
    n = arrs["output_kpts"].shape[DUMP_PAIR_AXIS["output_kpts"]]
    per_pair = sum(a.nbytes for a in arrs.values()) / n
    if per_pair * n > DUMP_BYTES:
        keep = np.sort(np.random.default_rng(seed).choice(n, max(1, int(DUMP_BYTES // per_pair)), replace=False))
        arrs = {k: np.take(a, keep, axis=DUMP_PAIR_AXIS.get(k, 0)) for k, a in arrs.items()}
        print(f"[bench] --dump-outputs: {len(keep)} of {n} pairs (seed {seed})", file=sys.stderr)
    os.makedirs(path, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


CONF_CFG = {(32, 1, 224, "dinov2_vits14"): "cfg1_", (32, 1, 256, "dinov2_vitb14"): "", (16, 5, 256, "dinov2_vitb14"): "cfg4_", (8, 1, 384, "dinov2_vitl14"): "cfg5_"}


def conformance_record(args, bs, S, H, arch, precision=None, head_precision=None):
    """The MEASURED conformance of a precision mode at scale (tools/conformance.py on the GPU box: >= 128 disjoint pairs x 2 weight seeds
    against the CPU oracle; committed under profiles/): argmax flips and the share of keypoints outside 1e-3 are rates of the mode,
    not of the 32-pair `parity_sample` of one run.  The newest record (r04 before r03) of the benched configuration, if any."""
    import glob
    precision, head_precision = precision or args.precision, head_precision or args.head_precision
    if (bs, S, H, arch) not in CONF_CFG:
        return None
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_conformance_{CONF_CFG[(bs, S, H, arch)]}{precision}_{head_precision}.json")))
    if not found:
        return None
    path = found[-1]
    d = json.load(open(path))
    from edgecape_amd import build
    if d.get("library_source_hash") != build.source_hash():
        # as pmc_traffic(): a record is a statement about ONE library; any kernel edit makes it stale until tools/conformance.py has run again
        return {"record": None, "reason": f"stale conformance record {os.path.relpath(path, ROOT)}: measured on library "
                                          f"{str(d.get('library_source_hash'))[:16]}, this is {build.source_hash()[:16]} (tools/gpu_conformance_all.sh)"}
    p = d["pooled"]
    rec = {"pairs": p["pairs"], "weight_seeds": [s_["weight_seed"] for s_ in d["per_weight_seed"]], "valid_keypoints": p["n_valid"],
           "argmax_flips": p["flips"], "flip_rate": p["flip_frac"], "max_abs_kpt_err": p["max_all"], "max_abs_kpt_err_flip_free": p["max_clean"],
           "p99_abs_kpt_err": p["p99"], "frac_gt_1e-3": p["frac_gt_1e3"], "pck@0.2_hip_vs_oracle_pred": p["pck_vs_oracle"], "tolerance": 1e-3,
           "source": os.path.relpath(path, ROOT)}
    g = p.get("near_tie_guard")
    if g:
        rec["near_tie_guard_2x_max_map_err"] = g["guards"]["2x_max"]
    return rec


def pmc_path(bs, S, H, arch, precision):
    """PMC summary of the north-star kernel for a workload: profiles/qkv_gemm_pmc.json for the headline configuration (cfg2, fp16),
    profiles/qkv_gemm_pmc_<arch>_<H>_b<bs>_s<S>_<precision>.json for any other (both written by tools/refresh_pmc.py)."""
    if (bs, S, H, arch, precision) == (32, 1, 256, "dinov2_vitb14", "fp16"):
        return os.path.join(ROOT, "profiles", "qkv_gemm_pmc.json")
    return os.path.join(ROOT, "profiles", f"qkv_gemm_pmc_{arch}_{H}_b{bs}_s{S}_{precision}.json")


def pmc_traffic(args, bs, S, H, arch, source_hash):
    """`traffic` cannot be measured from inside the process: it comes from the committed rocprofv3 --pmc summary of THIS command
    (profiles/qkv_gemm_pmc.json, written by tools/refresh_pmc.py on the GPU box: separate FETCH_SIZE / WRITE_SIZE passes, gfx950 x2
    read correction, MI355X_MICROARCH.md §HBM).  It is only reported when that summary was collected on this workload AND on this
    library: the summary carries the sha256 of the kernel sources it measured (edgecape_amd.build.source_hash); any edit of a
    kernel makes it stale and `traffic` null until tools/refresh_pmc.py is run again."""
    path = pmc_path(bs, S, H, arch, args.precision)
    if not os.path.exists(path):
        return {"traffic": None, "traffic_note": "no PMC summary (tools/refresh_pmc.py)"}
    d = json.load(open(path))
    if d.get("source_hash") != source_hash:
        return {"traffic": None, "traffic_note": f"stale PMC summary: collected on library {str(d.get('source_hash'))[:16]}, this is {source_hash[:16]}"}
    if d.get("workload") != [bs, S, H, arch, args.precision]:
        return {"traffic": None, "traffic_note": f"PMC summary is for workload {d.get('workload')}"}
    return {"traffic": d["traffic_bytes_per_launch"], "traffic_unit": "bytes/launch (L2 miss traffic incl. Infinity-Cache hits)",
            "algorithmic_bytes": d["algorithmic_bytes_per_launch"], "traffic_over_algorithmic": round(d["traffic_bytes_per_launch"] / d["algorithmic_bytes_per_launch"], 3),
            "mfma_util_pmc": d.get("mfma_util"), "traffic_source": os.path.relpath(path, ROOT)}


def episode_mode(args, sd, synth, bs, S, H, arch, apis, rank=0, world=1, n_ep=32, qpe=15, passes=6, n_img=0, precision=None, head_precision=None,
                 parity_episodes=0):
    """The reference's real evaluation protocol (not `value`): every support set is paired with 15 queries
    (EdgeCape/datasets/datasets/mp100/test_dataset.py:86-99), so `n_ep` episodes are `n_ep * 15` pairs.  Streamed through
    ec_forward_episodes: a call takes the next q queries of the pair order and encodes the episodes that start in it - their support
    images ride in the queries' backbone pass - with q chosen so that a call's backbone pass has about as many images as a headline
    step ((1 + S) * bs).  EVERY encode lies inside the timed region, amortised as the protocol amortises it; calls are pipelined
    (head of call i beside the backbone of call i + 1) with an ec_pipeline_flush inside the timed region (one un-overlapped head at the
    end of `passes` x n_ep episodes: 6 passes = 192 episodes = 2880 pairs, ~0.3 s - a test split of MP-100 is thousands).  Every rank streams its
    own n_ep episodes (weak scaling, as the headline); the region is apis.timed_steps' (barriers, max over ranks)."""
    import torch
    from edgecape_amd.engine import HipEngine
    from edgecape_amd.episodes import stream_schedule
    n_img = n_img or args.episode_images or (1 + S) * bs
    q = max(1, n_img * qpe // (qpe + S))
    cap = (q + qpe - 1) // qpe + 2
    eng = HipEngine(sd, arch=arch, image_size=H, max_batch=q, max_shots=S, backbone_precision=precision or args.precision,
                    head_precision=head_precision or args.head_precision)
    ep = np.repeat(np.arange(n_ep, dtype=np.int32), qpe)
    calls = stream_schedule(ep, q, cap)
    # synthetic data of the protocol's shape: n_ep support sets, and one pool of q query images that every call re-reads (distinct
    # pixels per call would only cost HBM; the work per call does not depend on them)
    sup = synth.make_pairs(n_ep, S, H, seed=3000, first_index=rank * n_ep, fixed_n_kp=False)
    qry = synth.make_pairs(q, 1, H, seed=4000, first_index=rank * q)
    mask = sup["target_weight_s"][0].copy()
    for tw in sup["target_weight_s"]:
        mask = mask * tw
    skels = [m["sample_skeleton"][0] for m in sup["img_metas"]]
    device = "cuda" if torch.cuda.is_available() else "cpu"
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    iq_all = dev(qry["img_q"])
    prepared = []
    for c in calls:
        new = None
        if len(c["new_episodes"]):
            e = np.asarray(c["new_episodes"])
            new = dict(img_s=[dev(x[e]) for x in sup["img_s"]], target_s=[dev(x[e]) for x in sup["target_s"]], mask_s=mask[e],
                       skeletons=[skels[i] for i in e], slots=c["new_slots"])
        prepared.append(eng.prepare_episode_call(iq_all[:len(c["queries"])], c["slot_of_query"], new))
    cache = eng.support_cache(cap)
    sets, count = {}, [0]

    def one_pass():
        for p in prepared:
            key = (p["bs"], count[0] & 1)
            count[0] += 1
            if key not in sets:
                sets[key] = eng._outputs(p["bs"])
            eng.forward_episodes(cache, prepared=p, outputs=sets[key], pipelined=True)

    def closing():
        eng.pipeline_flush()
        apis.allreduce_counts(np.zeros(6))

    dt = apis.timed_steps(one_pass, passes, 1, collective=closing)     # warm-up: one whole protocol pass
    n_calls, n_pairs = passes * len(prepared), passes * len(ep)
    imgs = len(ep) + n_ep * S
    parity = None
    if parity_episodes > 0 and rank == 0 and world == 1 and torch.cuda.is_available():
        # AFTER the timed region: the first call of the stream once more (it encodes its own episodes), and its first `parity_episodes`
        # episodes - the same support sets, the same query images as in every timed pass - against the CPU oracle on the expanded pairs
        # (the episode figure had no oracle-checked sample at its benched size)
        from oracle import edgecape_oracle as orc   # checker only
        outs = eng._outputs(prepared[0]["bs"])
        eng.forward_episodes(cache, prepared=prepared[0], outputs=outs, pipelined=True)
        eng.pipeline_flush()
        torch.cuda.synchronize()
        n_par = min(parity_episodes * qpe, len(calls[0]["queries"]))
        e = ep[calls[0]["queries"][:n_par]]
        pair_batch = dict(img_q=qry["img_q"][:n_par], img_s=[x[e] for x in sup["img_s"]], target_s=[x[e] for x in sup["target_s"]],
                          target_weight_s=[x[e] for x in sup["target_weight_s"]],
                          img_metas=[dict(qry["img_metas"][i], sample_skeleton=[skels[j]] * S) for i, j in enumerate(e)])
        torch.set_num_threads(min(16, max(1, physical_cores()[0])))
        _, ref = orc.forward_test(sd, pair_batch, synth.ARCHS[arch]["heads"])
        valid = (mask[:, :, 0] > 0)[e]
        got = outs[0]["output_kpts"].cpu().numpy()[:, :n_par]
        d_all = np.abs(got - ref["output_kpts"].numpy())
        am_g = outs[0]["similarity_map"].cpu().numpy()[:n_par].reshape(n_par, valid.shape[1], -1).argmax(-1)
        am_r = ref["similarity_map"].numpy().reshape(n_par, valid.shape[1], -1).argmax(-1)
        flips = (am_g != am_r) & valid
        clean = ~flips.any(axis=1)
        d = d_all[:, valid]
        d_clean = d_all[:, clean][:, valid[clean]] if clean.any() else np.zeros(1)
        parity = {"pairs": int(n_par), "episodes": int(len(set(e.tolist()))), "call": f"the stream's first call ({len(calls[0]['queries'])} queries + "
                  f"{len(calls[0]['new_episodes']) * S} support images), re-issued behind the timed region", "tolerance": 1e-3,
                  "max_abs_kpt_err_valid": float(d.max()), "max_abs_kpt_err_flip_free": float(d_clean.max()), "p99_abs_kpt_err_valid": float(np.quantile(d, 0.99)),
                  "frac_gt_1e-3": float((d > 1e-3).mean()), "argmax_flips": int(flips.sum()), "valid_keypoints": int(valid.sum()),
                  "within_tolerance": bool(d.max() < 1e-3), "oracle": "oracle/edgecape_oracle.py forward_test on the expanded (support set, query) pairs"}
    return {"value": round(world * n_pairs / dt, 2), **({"parity_sample": parity} if parity else {}), "unit": "images/s", "queries_per_episode": qpe, "episodes": n_ep, "pairs": len(ep), "shots": S,
            "queries_per_call": q, "calls_per_pass": len(prepared), "passes_timed": passes, "seconds": round(dt, 6), "ms_per_call": round(dt / n_calls * 1e3, 3),
            "backbone_images_per_pair": round(imgs / len(ep), 3), "backbone_images_per_pair_uncached": 1 + S,
            "entry_point": "ec_forward_episodes, pipelined; every encode inside the timed region",
            "note": "the reference's evaluation protocol (test_dataset.py:86-99): support side encoded once per episode (SURVEY 8f rank 1); not the headline metric"}


def physical_cores():
    """Physical cores this process may run on (one per set of SMT siblings inside the affinity mask)."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except Exception:
        allowed = list(range(os.cpu_count() or 1))
    seen = set()
    for c in allowed:
        try:
            sib = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
        except Exception:
            sib = str(c)
        seen.add(sib)
    return max(1, len(seen)), len(allowed)


def cpu_baseline(args, sd, eng, synth):
    """Time the CPU oracle (torch fp32 eager restatement of the reference, kind="port") on the host cores, BASELINE.md §4
    protocol: identical seeded pairs, 2 warm-ups + median of >= 5 timed forwards at bs = 2 and bs = 32, torch threads = physical
    cores unless a one-off sweep at bs = 2 (recorded) finds a faster count.  The bs = 32 batch doubles as the on-box parity sample
    of the HIP path (same pairs as rank 0's shard)."""
    import torch
    from oracle import edgecape_oracle as orc   # checker / baseline only — never the product path
    S, H, arch = args.shots, args.image_size, args.arch
    heads = synth.ARCHS[arch]["heads"]
    phys, logical = physical_cores()
    batches = [int(x) for x in args.cpu_batches.split(",") if x]
    small = synth.make_pairs(min(batches), S, H, seed=1000, fixed_n_kp=False)
    # thread sweep (one warm-up + one timed forward each): eager CPU kernels of this size stop scaling well below a two-socket core count
    sweep = {}
    cand = sorted({t for t in (8, 16, 32, 64, 96, phys) if t <= max(phys, 8)})
    for t in cand:
        torch.set_num_threads(t)
        orc.forward_test(sd, small, heads)
        t0 = time.perf_counter()
        orc.forward_test(sd, small, heads)
        sweep[t] = round(time.perf_counter() - t0, 4)
    threads = min(sweep, key=sweep.get)
    torch.set_num_threads(threads)
    per_bs = {}
    out = batch = None
    for n in batches:
        batch = small if n == min(batches) else synth.make_pairs(n, S, H, seed=1000, fixed_n_kp=False)
        for _ in range(2):
            res, out = orc.forward_test(sd, batch, heads)
        times = []
        for _ in range(max(args.cpu_runs, 1)):
            t0 = time.perf_counter()
            orc.forward_test(sd, batch, heads)
            times.append(time.perf_counter() - t0)
        per_bs[n] = {"pairs_per_s": round(n / float(np.median(times)), 3), "median_s": round(float(np.median(times)), 4), "runs": len(times)}
    n = batches[-1]
    # parity of the HIP path on the last (largest) batch: the first n pairs of rank 0's shard are exactly these pairs
    mask = batch["target_weight_s"][0].copy()
    for tw in batch["target_weight_s"]:
        mask = mask * tw
    o = eng.forward(batch["img_q"], batch["img_s"], batch["target_s"], mask, [m["sample_skeleton"][0] for m in batch["img_metas"]])
    torch.cuda.synchronize()
    valid = mask[:, :, 0] > 0
    got, ref = o["output_kpts"].cpu().numpy(), out["output_kpts"].numpy()
    d = np.abs(got - ref)[:, valid]
    sim_g = o["similarity_map"].cpu().numpy().reshape(n, 100, -1).argmax(-1)
    sim_r = out["similarity_map"].numpy().reshape(n, 100, -1).argmax(-1)
    flips = (sim_g != sim_r) & valid
    clean = ~flips.any(axis=1)                                   # samples without a proposal argmax flip (the reference's one discontinuity)
    d_clean = np.abs(got - ref)[:, clean][:, valid[clean]] if clean.any() else np.zeros(1)
    pred_g, pred_r = got[-1] * H, ref[-1] * H
    thr = 0.2 * H
    parity = {"pairs": n, "precision": args.precision, "head_precision": args.head_precision, "tolerance": 1e-3,
              "max_abs_kpt_err_valid": float(d.max()), "max_abs_kpt_err_flip_free": float(d_clean.max()),
              "p99_abs_kpt_err_valid": float(np.quantile(d, 0.99)), "median_abs_kpt_err_valid": float(np.median(d)),
              "frac_gt_1e-3": float((d > 1e-3).mean()), "argmax_flips": int(flips.sum()), "valid_keypoints": int(valid.sum()),
              # PCK@0.2 of the HIP predictions scored against the ORACLE's predictions (1.0 = every keypoint within 0.2 * bbox):
              # meaningful with random weights, unlike PCK against the synthetic ground truth (chance level for both)
              "pck@0.2_hip_vs_oracle_pred": round(float((np.linalg.norm(pred_g - pred_r, axis=-1)[valid] < thr).mean()), 4),
              "within_tolerance": bool(d.max() < 1e-3)}
    base = {"value": per_bs[n]["pairs_per_s"], "unit": "images/s", "cores": threads, "physical_cores": phys, "logical_cpus": logical,
            "kind": "port", "per_batch_size": {str(k): v for k, v in per_bs.items()},
            "thread_sweep_s_at_bs%d" % min(batches): {str(k): v for k, v in sweep.items()},
            "sample": f"{n} pairs ({S}-shot, {H}x{H}, {arch}) through oracle/edgecape_oracle.py forward_test, torch CPU fp32 eager, "
                      f"2 warm-ups + median of {max(args.cpu_runs, 1)} forwards, {threads} threads (fastest of the sweep; physical cores: {phys})"}
    return base, parity


if __name__ == "__main__":
    main()
