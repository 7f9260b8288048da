#!/usr/bin/env python3
"""The VQ-IMG training call (conf/img_config.yaml's model as bench.py builds it, 256 x 256 images, bf16 compute; the whole objective of
train.py:84-103: VQLPIPSWithDiscriminator with LPIPS on its HIP path and no face term, two Adams) in three forms, at B = 2 with accumulate 8
(the reference's own setting) and B = 32 with accumulate 1:

  eager               today's step: the loss's ATen tail, host-step Adams, the Codebook's host reservoir
  eager + HIP tail    hip_tail(True), Adam(device_step=True), the device reservoir: what the graph holds, issued launch by launch
  graphed             mas_hip.graphs.GraphedGanStep(accumulate=k) over the same

One model, loss and optimizer pair per column (same seed), the codebook in its steady phase (collect + lookup, no re-initialisation in
sight), the discriminator's gate open.  A block is n calls (a multiple of accumulate) between two device synchronisations, n sized from a
first short block to fill --seconds; the columns alternate block by block, two rounds.  The figure is device-synchronised wall time per CALL
(an optimizer step is `accumulate` calls).  The graphed column's block runs under torch.cuda.set_sync_debug_mode("error").  Launches per
call: the device activities torch.profiler records for one closing call (kernels and copies; "not measured" where the profiler gives none).

Then the tail alone, switch off against on, in the same process: the loss's two halves (discriminator passes included, no perceptual
term) on a reconstruction that is one 128 -> 3 convolution of a fixed map, forward and backward; device time (the sum of the profiler's
device activities) and their count per call, and the difference of the two columns, which is the tail's.

``--faces`` measures the face term inside the step INSTEAD: a synthetic-weight ``FaceLoss`` (tests/helpers/face_ref.py) on the loss, k faces
per call with k = 0, 1, 2 alternating as a data set would, in four columns that alternate block by block in one process:

  eager, lists             the step as it runs without this class: ATen tail, host-step Adams, the boxes as lists
  graphed, table           GraphedGanStep(images, bbox_face): the boxes through the step's FaceTable, the two variants per phase
  graphed, no faces        the same step called without boxes: the variant without the term, every call
  graphed, face_loss=None  the step as it was before the face term could be captured

then the face node alone, forward + backward at the batch's images: the list node against the fixed-capacity node at n = 1 and n = 3 faces
(2n rows forward and n backward against 6 and 3).

``--objects`` measures the object term inside the step INSTEAD: ``object_loss="lpips"`` on the loss (the perceptual LPIPS's weights), seeded
boxes of 48..160 px with 0 / 2 / 6 used crops per image alternating call by call, in columns that alternate block by block in one process:

  eager, lists           the step as it runs without this class: ATen tail, host-step Adams, the boxes as lists (the atlas cut to them)
  graphed, HxW[xN]       GraphedGanStep(images, None, bbox_obj) with an ObjectAtlas of that geometry: the default, one of twice its area
                         and, beyond B = 2, one scaled with the batch (a default canvas per two images); a call whose boxes do not fit
                         runs eagerly on the list path and counts in eager_calls

with the atlas efficiency (crop area / canvas area) of each box set on the fixed canvases and on the list path's own, then the object node
alone, forward + backward: the list node against the fixed-capacity node on each atlas the six-crop set fits."""
import argparse, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
os.environ.setdefault("MAS_LPIPS_STRICT", "0")          # LPIPS keeps its initialisation: timing does not depend on the weights' values
import torch
from mas_hip import graphs, ops, optim
from losses.loss_img import VQLPIPSWithDiscriminator, hip_tail
from losses.lpips import hip_path
from models import VQBASE
from models.modules import Conv2d

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0, help="wall time one timed block should fill")
ap.add_argument("--configs", default="2:8,32:1", help="batch:accumulate pairs")
ap.add_argument("--faces", action="store_true", help="measure the face term inside the step (see above) instead of the three forms")
ap.add_argument("--objects", action="store_true", help="measure the object term inside the step (see above) instead of the three forms")
a = ap.parse_args()

IMG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=3, out_channels=3, channels=[128, 128, 128, 256, 512, 512], num_res_blocks=2,
                             resolution=512, attn_resolutions=[32], dropout=0.0), n_embed=8192, embed_dim=256, init_steps=3000, reservoir_size=12500)
COLS = ("eager", "eager + HIP tail", "graphed")
dev = torch.device("cuda:0")
ops.set_compute_dtype(torch.bfloat16)


def device_activities(fn):
    """(count, total microseconds) of what torch.profiler records on the device for one fn(), or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return (len(ev), sum(e.time_range.elapsed_us() for e in ev)) if ev else None
    except Exception as e:                                    # a profiler that cannot trace this device: the times stand without the counts
        print(f"(profiler: {type(e).__name__}: {e})", flush=True)
        return None


def gan_call(model, crit, gopt, dopt, x, step, closing, last_layer=None, rec_fn=None, bbox_face=None, bbox_obj=None):
    rec, q = model(x) if rec_fn is None else rec_fn()
    d_loss = crit(1, step, x, rec)
    d_loss.backward()
    disc = list(crit.discriminator.parameters())
    for p in disc:
        p.requires_grad_(False)
    try:
        loss, _ = crit(0, step, x, rec, q, bbox_face=bbox_face, bbox_obj=bbox_obj, last_layer=last_layer if last_layer is not None else model.decoder.model[-1])
        loss.backward()
    finally:
        for p in disc:
            p.requires_grad_(True)
    if closing:
        dopt.step(); dopt.zero_grad(set_to_none=True)
        gopt.step(); gopt.zero_grad(set_to_none=True)
    return loss


def block(fn, n, guarded=False):
    torch.cuda.synchronize()
    if guarded:
        torch.cuda.set_sync_debug_mode("error")
    try:
        t0 = time.perf_counter()
        for _ in range(n):
            loss = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, loss


def face_boxes(batch, k):
    """k faces (0, 1 or 2) on the first images of a 256 x 256 batch: a portrait box and a landscape one"""
    boxes = [[] for _ in range(batch)]
    for i, box in enumerate(([40, 30, 168, 190], [96, 120, 240, 216])[:k]):
        boxes[i % batch].append(box)
    return boxes


def bench_faces():
    """--faces: the four step columns and the node alone, per configuration"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import face_ref
    from losses.face_loss import FaceLoss
    from mas_hip import face as FH
    ck = os.path.join(tempfile.mkdtemp(), "face_synth.pt")
    torch.save(face_ref.synth_face_state_dict(0), ck)
    os.environ["MAS_FACE_CKPT"] = ck
    names = ("eager, lists", "graphed, table", "graphed, no faces", "graphed, face_loss=None")
    for cfg in a.configs.split(","):
        batch, acc = (int(v) for v in cfg.split(":"))
        x = torch.rand(batch, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(dev)
        cycle = [face_boxes(batch, k) for k in (0, 1, 2)]
        cols = {}
        for name in names:
            torch.manual_seed(1)
            model = VQBASE(**IMG_CFG)
            with torch.no_grad():
                model.quantize.embedding.weight.normal_(0.0, 1.0)
            model = model.to(dev).train()
            model.quantize.q_counter = model.quantize.q_re_end
            crit = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss="lpips", face_loss=None if name.endswith("None") else FaceLoss()).to(dev)
            on = name != "eager, lists"
            if on:
                model.quantize.enable_device_reservoir(seed=7)
            gopt = optim.Adam(model.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            dopt = optim.Adam(crit.discriminator.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            if on:
                step = graphs.GraphedGanStep(model, crit, gopt, dopt, x, accumulate=acc, warmup=acc, global_step=0)
                boxed = name == "graphed, table"

                def call(step=step, boxed=boxed, n=[0]):
                    n[0] += 1
                    return step(x, cycle[n[0] % 3] if boxed else None).loss
                for _ in range(3 * acc):
                    call()
                print(f"B={batch} accumulate={acc} {name}: {step.captures} capture(s)", flush=True)
            else:
                def call(model=model, crit=crit, gopt=gopt, dopt=dopt, n=[0]):
                    n[0] += 1
                    with hip_tail(False):
                        return gan_call(model, crit, gopt, dopt, x, n[0], n[0] % acc == 0, bbox_face=cycle[n[0] % 3])
                for _ in range(3 * acc):
                    call()
            cols[name] = call
        unit = 3 * acc                                            # a block holds whole cycles of the boxes and whole optimizer steps
        n_calls = {k: max(1, int(a.seconds / block(fn, unit, k != names[0])[0]) // unit) * unit for k, fn in cols.items()}
        times = {k: [] for k in cols}
        for _ in range(2):
            for k, fn in cols.items():
                dt, loss = block(fn, n_calls[k], k != names[0])
                assert bool(torch.isfinite(loss)), (k, float(loss))
                times[k].append(dt)
        for k in cols:
            print(f"VQ-IMG 256x256 B={batch} accumulate={acc} training call, faces 0/1/2 alternating, {k}: "
                  + " / ".join(f"{t * 1e3:.2f}" for t in times[k]) + f" ms/call ({n_calls[k]} calls per block)", flush=True)
        del cols, model, gopt, dopt, step, crit
        torch.cuda.empty_cache()

        # ---- the node alone: lists (2n rows forward, n backward) against the table (6 and 3) ---------------------------------------------------
        mod = FaceLoss().to(dev)
        rec = (x + 0.1 * torch.randn_like(x)).clamp(0, 1)
        table = FH.FaceTable(dev)
        three = [[[40, 30, 168, 190], [96, 120, 240, 216], [10, 10, 120, 130]]] + [[] for _ in range(batch - 1)]
        for n, boxes in ((1, face_boxes(batch, 1)), (3, three)):
            assert table.write(boxes, batch) == n
            res = {}
            for _ in range(2):
                for k, bb in (("lists", boxes), ("table", table)):
                    def node(bb=bb):
                        r = rec.clone().requires_grad_(True)
                        loss = mod(x, r, bb)
                        loss.backward()
                        return loss
                    for _ in range(3):
                        node()
                    res.setdefault(k, []).append((device_activities(node), block(node, 30)[0]))
            for k in ("lists", "table"):
                print(f"face node alone B={batch} n={n}, {k}: " + " / ".join(
                    (f"{c[0]} device activities, {c[1] / 1e3:.3f} ms on the device" if c else "device activities not measured") + f", {t * 1e3:.3f} ms wall"
                    for c, t in res[k]), flush=True)
        del mod, rec, table
        torch.cuda.empty_cache()


def object_boxes(batch, per_image, seed):
    """``per_image`` seeded boxes of 48..160 px on every image of a 256 x 256 batch, some partly outside it"""
    import random
    rng = random.Random(seed)
    out = []
    for _ in range(batch):
        boxes = []
        for _ in range(per_image):
            h, w = rng.randint(48, 160), rng.randint(48, 160)
            y0, x0 = rng.randint(-h // 4, 256 - 3 * h // 4), rng.randint(-w // 4, 256 - 3 * w // 4)
            boxes.append([x0, y0, x0 + w, y0 + h])
        out.append(boxes)
    return out


def bench_objects():
    """--objects: the step columns and the node alone, per configuration"""
    import warnings
    from mas_hip import objects as O
    for cfg in a.configs.split(","):
        batch, acc = (int(v) for v in cfg.split(":"))
        x = torch.rand(batch, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(dev)
        cycle = [object_boxes(batch, k, 10 + k) for k in (0, 2, 6)]
        atlases = {"544x1088": dict(), "1088x1088": dict(height=1088)}
        if batch > 2:
            atlases[f"544x1088x{batch // 2}"] = dict(canvases=batch // 2, max_cells=6 * batch)
        for name, kw in atlases.items():
            probe = O.ObjectAtlas("cpu", batch, **kw)
            eff = []
            for boxes in cycle[1:]:
                if probe.fits(boxes):
                    probe.write(boxes)
                eff.append(f"{probe.efficiency():.3f}" if probe.fits(boxes) else "does not fit")
            print(f"B={batch} atlas {name}: efficiency (crop area / canvas area) at 2 / 6 crops per image: {' / '.join(eff)}", flush=True)
        tight = [O.make_plan(boxes, batch) for boxes in cycle[1:]]
        print(f"B={batch} list path's own canvases: " + " / ".join(f"{p.n_canvas} x {p.H} x {p.W}, efficiency {p.efficiency():.3f}" for p in tight), flush=True)
        names = ("eager, lists",) + tuple(f"graphed, {k}" for k in atlases)
        cols, steps = {}, {}
        for name in names:
            torch.manual_seed(1)
            model = VQBASE(**IMG_CFG)
            with torch.no_grad():
                model.quantize.embedding.weight.normal_(0.0, 1.0)
            model = model.to(dev).train()
            model.quantize.q_counter = model.quantize.q_re_end
            crit = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss="lpips", face_loss=None, object_loss="lpips").to(dev)
            on = name != names[0]
            if on:
                model.quantize.enable_device_reservoir(seed=7)
            gopt = optim.Adam(model.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            dopt = optim.Adam(crit.discriminator.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            if on:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    step = graphs.GraphedGanStep(model, crit, gopt, dopt, x, accumulate=acc, warmup=acc, global_step=0,
                                                 object_atlas=atlases[name[len("graphed, "):]])

                    def call(step=step, n=[0]):
                        n[0] += 1
                        return step(x, None, cycle[n[0] % 3]).loss
                    for _ in range(3 * acc):
                        call()
                steps[name] = step
                print(f"B={batch} accumulate={acc} {name}: {step.captures} capture(s)", flush=True)
            else:
                def call(model=model, crit=crit, gopt=gopt, dopt=dopt, n=[0]):
                    n[0] += 1
                    with hip_tail(False):
                        return gan_call(model, crit, gopt, dopt, x, n[0], n[0] % acc == 0, bbox_obj=cycle[n[0] % 3])
                for _ in range(3 * acc):
                    call()
            cols[name] = call
        unit = 3 * acc                                            # a block holds whole cycles of the boxes and whole optimizer steps
        guarded = {k: k in steps and all(steps[k].object_atlas.fits(b) for b in cycle) for k in cols}     # (an eager call reads on the host)
        n_calls = {k: max(1, int(a.seconds / block(fn, unit, guarded[k])[0]) // unit) * unit for k, fn in cols.items()}
        times = {k: [] for k in cols}
        before = {k: s.eager_calls for k, s in steps.items()}
        for _ in range(2):
            for k, fn in cols.items():
                dt, loss = block(fn, n_calls[k], guarded[k])
                assert bool(torch.isfinite(loss)), (k, float(loss))
                times[k].append(dt)
        for k in cols:
            extra = f", eager_calls {steps[k].eager_calls - before[k]} of {2 * n_calls[k]}" if k in steps else ""
            print(f"VQ-IMG 256x256 B={batch} accumulate={acc} training call, crops per image 0/2/6 alternating, {k}: "
                  + " / ".join(f"{t * 1e3:.2f}" for t in times[k]) + f" ms/call ({n_calls[k]} calls per block{extra})", flush=True)
        lp = crit.object_loss.net
        del cols, steps, model, gopt, dopt, step, crit
        torch.cuda.empty_cache()

        # ---- the node alone: the list node (a canvas cut to the boxes) against the fixed-capacity node on each atlas ------------------------
        rec = (x + 0.1 * torch.randn_like(x)).clamp(0, 1)
        for per, boxes in ((2, cycle[1]), (6, cycle[2])):
            tables = {"lists": boxes}
            for name, kw in atlases.items():
                atlas = O.ObjectAtlas(dev, batch, **kw)
                if atlas.fits(boxes):
                    atlas.write(boxes)
                    tables[name] = atlas
            res = {}
            for _ in range(2):
                for k, bb in tables.items():
                    def node(bb=bb):
                        r = rec.clone().requires_grad_(True)
                        out = (O.object_loss_static if isinstance(bb, O.ObjectAtlas) else O.object_loss)(lp, x, r, bb)
                        out[0].backward()
                        return out[0]
                    for _ in range(3):
                        node()
                    res.setdefault(k, []).append(block(node, 20)[0])
            for k in tables:
                print(f"object node alone B={batch}, {per} crops per image, {k}: " + " / ".join(f"{t * 1e3:.3f}" for t in res[k]) + " ms wall", flush=True)
        del lp, rec, tables
        torch.cuda.empty_cache()


with hip_path(True):
    if a.faces:
        bench_faces()
    if a.objects:
        bench_objects()
    for cfg in ([] if a.faces or a.objects else a.configs.split(",")):
        batch, acc = (int(v) for v in cfg.split(":"))
        x = torch.rand(batch, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(dev)
        cols, counts = {}, {}
        for name in COLS:
            torch.manual_seed(1)
            model = VQBASE(**IMG_CFG)
            with torch.no_grad():
                model.quantize.embedding.weight.normal_(0.0, 1.0)
            model = model.to(dev).train()
            model.quantize.q_counter = model.quantize.q_re_end          # steady state: collect + lookup, no k-means
            crit = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss="lpips", face_loss=None).to(dev)
            on = name != "eager"
            if on:
                model.quantize.enable_device_reservoir(seed=7)
            gopt = optim.Adam(model.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            dopt = optim.Adam(crit.discriminator.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            if name == "graphed":
                torch.cuda.synchronize(); t0 = time.perf_counter()
                step = graphs.GraphedGanStep(model, crit, gopt, dopt, x, accumulate=acc, warmup=acc, global_step=0)
                for _ in range(acc):
                    step(x)
                torch.cuda.synchronize()
                print(f"B={batch} accumulate={acc} graphed: {acc} warm-up calls + {step.captures} capture(s) + {acc} replays "
                      f"{time.perf_counter() - t0:.2f} s", flush=True)
                cols[name] = lambda step=step: step(x).loss
            else:
                def eager(model=model, crit=crit, gopt=gopt, dopt=dopt, on=on, n=[0]):
                    n[0] += 1
                    with hip_tail(on):
                        return gan_call(model, crit, gopt, dopt, x, n[0], n[0] % acc == 0)
                for _ in range(2 * acc):
                    eager()
                cols[name] = eager
            for _ in range(acc - 1):                          # the profiled call is a closing one
                cols[name]()
            counts[name] = device_activities(cols[name])
        n_calls = {k: max(2, int(a.seconds / block(fn, acc, k == "graphed")[0]) // acc) * acc for k, fn in cols.items()}
        times = {k: [] for k in cols}
        for _ in range(2):
            for k, fn in cols.items():
                dt, loss = block(fn, n_calls[k], k == "graphed")
                assert bool(torch.isfinite(loss)), (k, float(loss))
                times[k].append(dt)
        for k in cols:
            c = counts[k]
            print(f"VQ-IMG 256x256 B={batch} accumulate={acc} training call, {k}: " + " / ".join(f"{t * 1e3:.2f}" for t in times[k])
                  + f" ms/call ({n_calls[k]} calls per block)  best {batch / min(times[k]):.1f} images/s; device activities of a closing call: "
                  + (f"{c[0]} ({c[1] / 1e3:.2f} ms)" if c else "not measured"), flush=True)
        del cols, model, gopt, dopt, step, crit
        torch.cuda.empty_cache()

        # ---- the tail alone: the loss's two halves on a reconstruction that is one convolution of a fixed map ---------------------------------
        torch.manual_seed(2)
        last = Conv2d(128, 3, 3, 1, 1).to(dev)
        h = torch.randn(batch, 128, 256, 256, generator=torch.Generator().manual_seed(3)).to(dev)
        crit = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None).to(dev)
        q = torch.zeros((), device=dev)
        res = {}
        for on in (False, True, False, True):
            def tail(on=on):
                with hip_tail(on):
                    loss = gan_call(None, crit, None, None, x, 1, False, last_layer=last, rec_fn=lambda: (last(h), q))
                last.zero_grad(set_to_none=True); crit.zero_grad(set_to_none=True)
                return loss
            for _ in range(3):
                tail()
            res.setdefault(on, []).append((device_activities(tail), block(tail, 20)[0]))
        for on in (False, True):
            print(f"loss call (discriminator passes + tail) B={batch}, hip_tail {'on' if on else 'off'}: " + " / ".join(
                (f"{c[0]} device activities, {c[1] / 1e3:.3f} ms on the device" if c else "device activities not measured") + f", {t * 1e3:.3f} ms wall"
                for c, t in res[on]), flush=True)
        if all(c for v in res.values() for c, _ in v):
            d_n = res[False][-1][0][0] - res[True][-1][0][0]
            d_t = min(c[1] for c, _ in res[False]) - min(c[1] for c, _ in res[True])
            print(f"  the HIP tail: {d_n} fewer device activities and {d_t / 1e3:.3f} ms less device time per call at B={batch}", flush=True)
        del last, h, crit
        torch.cuda.empty_cache()
