#!/usr/bin/env python3
"""Image-token sampling on the MI355X: ``MakeAScene.generate`` eager against ``graph=True`` (one captured decode step replayed per
token, models/decode_graph.py) at config-4 width -- 24 layers, hidden 1024, 16 heads, 256 text + 16x16 seg + 32x32 image tokens, image
vocabulary 8192, random weights -- under bf16 autocast, B in {1, 8}, with and without classifier-free guidance (cond_scale 3.0).
Temperature 1, top_k 256.  One JSON line.

    python tools/sample_bench.py [--batch 1 8] [--runs 2] [--skip-eager] [--kv-splits 2 4 8 16 auto]
    python tools/sample_bench.py --profile [--kv-splits 8]   # one graph-path call per split count after a warm one: run it under
                                                             # rocprofv3 --kernel-trace --stats
    python tools/sample_bench.py --skip-eager --kv-splits 8 --top-p 0.9   # beside every graph column the same call with top_p
    python tools/sample_bench.py --skip-eager --kv-splits 8 --keep-rows 0 16   # image prompts: the top N token rows of a random image kept

``--kv-splits``: beside the unsplit decode attention, the graph path with ``generate(kv_splits=n)`` for every n given (integers or
"auto"): ``graph_ms_per_token_kv<n>`` columns, measured in the same process, every run alternating over the columns.  With
``--profile`` the unsplit call and one call per n run back to back, so one trace holds ``attn_decode_dev_kernel`` beside
``attn_decode_split_partial_kernel`` / ``attn_decode_split_combine_kernel`` with 24 * 1023 calls each.

``--top-p P``: ``generate(top_p=P)`` next to every graph-path column (``..._topp`` keys), alternating with it in the same runs; with
``--profile`` every call is followed by its top_p twin, so the trace's ``sample_kernel`` rows hold both (the per-call wall times tell
them apart; the kernel statistics of a run with and one without ``--top-p`` give the sampler's own times).

``--keep-rows N ...``: ``generate(img_tokens=random image, keep=its top N token rows)`` next to every graph-path column, once with
``prefill_prefix`` on (``..._keep<N>`` keys: the kept rows go through the prefill, 1023 - 32 N replays) and once off (``..._keep<N>_steps``:
every position is a decode step), alternating with the unprompted call in the same runs.  N = 0 keeps nothing: the prompted sampler
entry on the unprompted amount of work.  The mask is a CPU tensor (no synchronisation to find the prefix).  ms per token stays the
call time / 1024 whatever is kept, so the columns compare as call times.  With ``--profile`` every call is followed by its prompted
twins (``prefill_prefix`` off: 1023 more ``sample_kernel`` launches with the mask).

``--num-samples N ...``: a section of its own (the others are skipped): ``generate(num_samples=N, graph=True)`` for B = 1 prompt, plain
and guided, ``--kv-splits`` as given (the first one; default "auto").  Columns ``expanded`` (``share_prompt=False``: the prompts
repeated, the path a call on ``text.expand(N, -1)`` takes) and ``shared`` (``share_prompt=True``: one prefill, the prompt's K / V stored
once, ``mas_attn_decode_shared_dev``), timed in one process, twice each (more with ``--runs``), alternating; ms per token (call time /
1024: one token of all N candidates) and ``torch.cuda.max_memory_allocated`` of a call of each column alone.  ``--prompt-splits P ...``
adds ``shared_p<P>`` columns with the prompt block in P key ranges instead of ``decode.resolve_prompt_splits("auto", ...)``.  With
``--profile``: one guided call per column after a warm one, for rocprofv3 --kernel-trace --stats.

ms per token = wall time of a whole call (prefill, first token and the 1023 replays, synchronised) / 1024; capture = first graph call
minus a steady one (warm-up step, capture, graph instantiation)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

CFG = dict(num_layers=24, hidden_dim=1024, num_attn_heads=16, image_vocab_size=8192, seg_vocab_size=256, text_vocab_size=16384,
           image_tokens_per_dim=32, seg_tokens_per_dim=16, text_length=256)


def build(dev):
    from models.transformer import MakeAScene
    torch.manual_seed(0)
    m = MakeAScene(**CFG).to(dev).eval()
    return m


def prompt(b, dev):
    g = torch.Generator().manual_seed(b)
    text = torch.randint(1, CFG["text_vocab_size"] - CFG["text_length"], (b, CFG["text_length"]), generator=g)
    text[:, 200:] = 0
    seg = torch.randint(0, CFG["seg_vocab_size"], (b, CFG["seg_tokens_per_dim"] ** 2), generator=g)
    return text.to(dev), seg.to(dev)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def num_samples_section(a, m, dev, L, kw):
    """--num-samples: B = 1 prompt, n candidates, plain and guided; columns ``share_prompt=False`` (the prompts expanded: the path of a
    call on ``text.expand(n, -1)``), ``True`` and, with --prompt-splits, ``True`` with a fixed prompt split count"""
    from mas_hip import decode
    text, seg = prompt(1, dev)
    kvs = a.kv_splits[0] if a.kv_splits else "auto"
    auto_rule = decode.resolve_prompt_splits
    cols = [("expanded", False, None), ("shared", True, None)] + [(f"shared_p{p}", True, p) for p in a.prompt_splits]

    def call(n, cs, share, psplit):
        decode.PROMPT_SPLITS_OVERRIDE = psplit              # None: "auto" (generate() has no argument for the prompt split count)
        try:
            return m.generate(text, seg, cond_scale=cs, graph=True, kv_splits=kvs, num_samples=n, share_prompt=share, **kw)
        finally:
            decode.PROMPT_SPLITS_OVERRIDE = None

    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if a.profile:
        res = {"B": 1, "cond_scale": 3.0, "kv_splits": kvs}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for n in a.num_samples:
                for tag, share, psplit in cols:
                    call(n, 3.0, share, psplit)
                    res[f"profile_call_s_n{n}_{tag}"] = round(timed(lambda: call(n, 3.0, share, psplit))[0], 4)
        print(json.dumps(res))
        return
    rows = []
    for n in a.num_samples:
        for cs in (None, 3.0):
            groups = 2 if cs is not None else 1
            r = {"B": 1, "num_samples": n, "cond_scale": cs, "kv_splits": kvs, "kv_resolves_to": m._resolve_kv_splits(kvs, groups * n),
                 "prompt_splits_auto": auto_rule("auto", groups, n, CFG["num_attn_heads"], cus)}
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                for tag, share, psplit in cols:                     # memory: each column alone, entries and cached blocks released first
                    m.release_decode_graphs()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    call(n, cs, share, psplit)
                    torch.cuda.synchronize()
                    r[f"max_memory_allocated_MiB_{tag}"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
                m.release_decode_graphs()
                for tag, share, psplit in cols:                     # capture
                    call(n, cs, share, psplit)
                times = {c[0]: [] for c in cols}
                for _ in range(max(2, a.runs)):                     # every column twice, alternating: the spread is the noise to beat
                    for tag, share, psplit in cols:
                        times[tag].append(timed(lambda: call(n, cs, share, psplit))[0])
            for tag, _, _ in cols:
                r[f"ms_per_token_{tag}"] = round(1e3 * min(times[tag]) / L, 4)
                r[f"spread_ms_per_token_{tag}"] = round(1e3 * (max(times[tag]) - min(times[tag])) / L, 4)
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            m.release_decode_graphs()
    print(json.dumps({"metric": "MakeAScene.generate(num_samples=n), config-4 width, bf16 autocast", "tokens_per_image": L,
                      "top_k": kw["top_k"], "device": torch.cuda.get_device_name(0), "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kv-splits", nargs="+", default=[], type=lambda v: v if v == "auto" else int(v),
                    help="also time generate(graph=True, kv_splits=n) for every n given (integers or 'auto')")
    ap.add_argument("--top-p", type=float, default=None, help="also time every graph-path column with generate(top_p=P)")
    ap.add_argument("--keep-rows", type=int, nargs="+", default=[],
                    help="also time every graph-path column with the top N token rows of a random image kept, prefill_prefix on and off")
    ap.add_argument("--num-samples", type=int, nargs="+", default=[],
                    help="time generate(num_samples=N, graph=True) for one prompt: share_prompt False against True (this section only)")
    ap.add_argument("--prompt-splits", type=int, nargs="+", default=[],
                    help="with --num-samples: also the shared column with the prompt block in this many key ranges instead of 'auto'")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = build(dev)
    L = CFG["image_tokens_per_dim"] ** 2
    kw = dict(temperature=1.0, top_k=256)
    n_dim = CFG["image_tokens_per_dim"]
    if any(not 0 <= n <= n_dim for n in a.keep_rows):
        ap.error(f"--keep-rows: 0 .. {n_dim}")

    def prompt_kw(b, pk):
        """generate's image-prompt arguments of a column: pk = None (unprompted) or (kept token rows, prefill_prefix)"""
        if pk is None:
            return {}
        from models import border_keep_mask
        img = torch.randint(0, CFG["image_vocab_size"], (b, L), generator=torch.Generator().manual_seed(100 + b)).to(dev)
        return dict(img_tokens=img, keep=border_keep_mask(n_dim, up=pk[0])[None].repeat(b, 1), prefill_prefix=pk[1])

    if a.num_samples:
        num_samples_section(a, m, dev, L, kw)
        return
    prompts = [None] + [(n, on) for n in a.keep_rows for on in (True, False)]
    ptag = lambda pk: "" if pk is None else f"_keep{pk[0]}" + ("" if pk[1] else "_steps")
    if a.profile:
        text, seg = prompt(1, dev)
        res = {"B": 1, "cond_scale": 3.0}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for n in [None] + a.kv_splits:
                for tp in [None] + ([a.top_p] if a.top_p is not None else []):
                    for pk in prompts:
                        pkw = prompt_kw(1, pk)
                        m.generate(text, seg, cond_scale=3.0, graph=True, kv_splits=n, top_p=tp, **kw, **pkw)
                        dt, _ = timed(lambda: m.generate(text, seg, cond_scale=3.0, graph=True, kv_splits=n, top_p=tp, **kw, **pkw))
                        res[("profile_call_s" if n is None else f"profile_call_s_kv{n}") + ("" if tp is None else "_topp") + ptag(pk)] = round(dt, 4)
        print(json.dumps(res))
        return
    rows = []
    for b in a.batch:
        text, seg = prompt(b, dev)
        for cs in (None, 3.0):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                first, _ = timed(lambda: m.generate(text, seg, cond_scale=cs, graph=True, **kw))
                g = min(timed(lambda: m.generate(text, seg, cond_scale=cs, graph=True, **kw))[0] for _ in range(a.runs))
                e = None if a.skip_eager else min(timed(lambda: m.generate(text, seg, cond_scale=cs, **kw))[0] for _ in range(max(1, a.runs - 1)))
            r = {"B": b, "cond_scale": cs, "graph_ms_per_token": round(1e3 * g / L, 4), "graph_images_per_min": round(60 * b / g, 2),
                 "capture_s": round(first - g, 3)}
            if a.kv_splits or a.top_p is not None or a.keep_rows:
                # every column twice (more with --runs), alternating over the columns: the spread of the repeats is the noise to beat
                cols = [(n, tp, pk) for n in [None] + a.kv_splits for tp in [None] + ([a.top_p] if a.top_p is not None else [])
                        for pk in prompts]
                pkws = {pk: prompt_kw(b, pk) for pk in prompts}
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    for n, tp, pk in cols[1:]:
                        m.generate(text, seg, cond_scale=cs, graph=True, kv_splits=n, top_p=tp, **kw, **pkws[pk])          # capture
                    times = {c: [] for c in cols}
                    for _ in range(max(2, a.runs)):
                        for n, tp, pk in cols:
                            times[(n, tp, pk)].append(timed(lambda: m.generate(text, seg, cond_scale=cs, graph=True, kv_splits=n, top_p=tp,
                                                                               **kw, **pkws[pk]))[0])
                for n, tp, pk in cols:
                    tag = ("none" if n is None else str(n)) + ("" if tp is None else "_topp") + ptag(pk)
                    r[f"graph_ms_per_token_kv{tag}"] = round(1e3 * min(times[(n, tp, pk)]) / L, 4)
                    r[f"spread_ms_per_token_kv{tag}"] = round(1e3 * (max(times[(n, tp, pk)]) - min(times[(n, tp, pk)])) / L, 4)
                if a.kv_splits:
                    r["kv_auto_resolves_to"] = m._resolve_kv_splits("auto", 2 * b if cs is not None else b)
            if e is not None:
                r.update(eager_ms_per_token=round(1e3 * e / L, 4), eager_images_per_min=round(60 * b / e, 2), speedup=round(e / g, 2))
            rows.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
            m.release_decode_graphs()
    print(json.dumps({"metric": "MakeAScene.generate, config-4 width, bf16 autocast", "tokens_per_image": L, "top_k": kw["top_k"], "top_p": a.top_p, "keep_rows": a.keep_rows,
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
