"""The vector quantiser's lookup and its gradients, row by row and element by element against fp64.

The rest of the suite judges the lookup on Gaussian operands, whose top-2 gap is thousands of times the fp32 noise, by one number per
tensor: no exact tie ever occurs, no split is ever empty, D = 128 never reaches vq_finalize or a backward kernel, one wrong code row
beside 8191 right ones passes, and the atomics path (MAS_VQ_BWD_DET=0) is not run at all.  Here tests/helpers/vq_elementwise_check.py
runs, in one child process per setting (the switch is read once per process), row_sqnorm + vq_partial<32 / 64 / 128 / 256> +
vq_finalize + vq_loss_reduce through ``ops.vq_lookup`` at shapes with empty trailing splits, a split count capped by 1024 / row blocks,
two tiles per split with a ragged last tile and degenerate sizes, and vq_bwd_kernel + vq_bwd_codebook_kernel (``default``) resp.
vq_bwd_kernel with atomics (``atomic``) through autograd and through ``mas_vq_bwd`` itself, and records every output.  All judging is on
the CPU (``judge`` in the helper; every bound is derived in the helper's docstring from the kernels' arithmetic):

  * gauss / far: z, cb ~ N(0, 1), far shifted by +8 (+3 at D = 256) so that |z|^2 + |e|^2 is some 60 times the distances.  Per row:
    d64[idx] - min d64 <= B(idx) + B(argmin) always, idx EQUAL to the fp64 argmin where the top-2 gap exceeds the bound (every gauss
    row, at least 90 % of the far rows of each case), z_q bitwise cb[idx], the loss inside its chain bound;
  * int: integers in [-4, 4], every fp32 value exact: idx equal to the FIRST fp64 minimum on every row, with ties planted in every
    relation the merge order has (adjacent registers of a lane, the two half-waves, successive tiles of a split, adjacent splits, first
    against last active split, code 0 against code K - 1, a triple across three splits); z_q bitwise; a second lookup of z_q returns
    the same idx and z_q;
  * non-finite latent rows (three all-NaN, one with a single NaN, one with +inf, one with -inf): every idx in [0, K), z_q bitwise
    cb[idx], all other rows bitwise those of the call with finite rows, the loss non-finite;
  * backward, z = cb[pick] + 0.01 randn so that the test controls idx: all M rows on one code, hits exactly at the wave-quarter and
    64-wide ballot boundaries, picked codes in the ragged last 8-group, M in {1, 3}, random collisions; the three argument shapes of
    ``_VQ.backward``; ``mas_vq_bwd`` on a dcb pre-filled with NaN (every row stored, unpicked rows exactly 0) and with ones (the atomics
    path adds to them: the witness of which path ran, beside ``ops.last_kernel()``); dz and dcb per element inside their bounds, a
    second run bitwise equal (``default``), and with integer operands and power-of-two M D, g_loss, beta bitwise the fp64 result in
    both settings.

REQUIRED lists the (kernel, feature) pairs the children have to reach; a dispatch change that leaves a case vacuous fails here.

Measured worst |error| / bound on an MI355X (1 = the bound):
  index slack   (d64[idx] - min d64) / (B(idx) + B(argmin)): 0.000 in gauss, far and int alike -- the kernels took the fp64 argmin on
                EVERY row, the rows inside the bound included.  Rows judged by the slack rule alone (far; none in gauss): 130x2080x32
                1 of 130, 33x2049x256 2 of 33, 2049x1985x32 16 of 2049, 161x100x64 2 of 161, 97x161x128 6 of 97, 129x257x256 and the
                three degenerate sizes 0
  loss          gauss 0.080, far 0.112, int 0.664 (of the two roundings of the scale)
  dz            gauss 0.499 in both settings (one fma: half of what the bound allows for a product and a sum); int: bitwise
  dcb           fixed order gauss 0.335, atomics gauss 0.383; int: bitwise in both settings; a second run of the fixed order is bitwise
                equal; over a NaN fill every row is finite and the unpicked rows are 0.0, over ones the atomics path leaves 1.0 there
  int mode: every index is the first fp64 minimum, every planted tie of every relation resolves to the lower code, the second lookup
  of z_q returns the same idx and z_q; the six non-finite rows take code 0, all other rows are bitwise those of the finite call.
Every figure equals what the helper's fp32 numpy model gives for the same operands.  No kernel defect was found.  The three tests take
~8 s together on an MI355X box (two children, ~3 s each, most of it the interpreter's start)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import vq_elementwise_check as CHK  # noqa: E402

CHILD = os.path.join(HERE, "helpers", "vq_elementwise_check.py")
CHILD_TIMEOUT = 240
SWITCHES = ("MAS_VQ_BWD_DET",)
_WIDTHS = {"D32", "D64", "D128", "D256"}
_PATTERNS = {"one", "edges", "ragged", "small", "rand16", "need_z", "need_cb", "need_both", "int_exact"}
REQUIRED = {
    "forward": ("default", {
        "vq_partial": _WIDTHS | {"empty_splits", "ksplit_capped", "two_tiles_ragged", "one_split", "row_blocks_17"},
        "vq_finalize": {"tie:" + r for r in CHK.TIE_RELATIONS} | {"idempotent", "nonfinite"},
    }),
    "backward": ("default", {"vq_bwd_codebook": _WIDTHS | _PATTERNS | {"prefill_overwritten"}}),
    "atomics": ("atomic", {"vq_bwd": _WIDTHS | _PATTERNS | {"prefill_added_to"}}),
}
_children = {}          # label -> loaded recording, or an error text: a child runs once per session, and after a failure none is started


def _child(label, tmp_path_factory):
    broken = [v for v in _children.values() if isinstance(v, str)]
    if broken:
        pytest.fail("an earlier child failed; no further child is started\n" + broken[0][:2000])
    if label not in _children:
        extra = next(e for s, e, _ in CHK.SETTINGS if s == label)
        env0 = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        out = str(tmp_path_factory.mktemp("vq") / f"vq_{label}.pt")
        try:
            p = subprocess.run([sys.executable, CHILD, label, out], env={**env0, **extra}, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            if p.returncode != 0:
                _children[label] = f"child {label} exited with {p.returncode}\n{p.stdout}\n{p.stderr[-6000:]}"
            else:
                _children[label] = torch.load(out)
        except subprocess.TimeoutExpired as e:
            _children[label] = f"child {label} timed out after {CHILD_TIMEOUT} s\n{e.stdout or ''}\n{e.stderr or ''}"
    if isinstance(_children[label], str):
        pytest.fail(_children[label])
    return _children[label]["results"]


def _judge_all(part, cases, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    label, required = REQUIRED[part]
    got = _child(label, tmp_path_factory)
    failures, worst, reached = [], {}, set()
    for c in cases:
        for mode in CHK.modes_of(c):
            rows, r, f, notes = CHK.judge(c, mode, got[(c["name"], mode)], label)
            reached |= r
            failures += f
            for key, fam, fig, verdict in rows:
                print(f"{label:8s} {c['name']:20s} {mode:5s} {key:40s} {fam:24s} {fig:>10s} {verdict}")
                if verdict != "equal":
                    worst[fam] = max(worst.get(fam, 0.0), float(fig))
            if "slack_only" in notes:
                print(f"{label:8s} {c['name']:20s} {mode:5s} rows judged by the slack rule alone: {notes['slack_only']} of {c['M']}")
    print(f"worst |error| / bound per family, {part}:")
    for fam in sorted(worst):
        print(f"  {fam:32s} {worst[fam]:.3f}")
    for kern, want in required.items():
        missing = sorted(f for f in want if (kern, f) not in reached)
        if missing:
            failures.append(f"{kern}: the {label} child did not reach {missing}")
    assert not failures, "\n".join(failures[:60])


def test_lookup_row_by_row_vs_fp64(tmp_path_factory):
    _judge_all("forward", CHK.FWD_CASES + [CHK.NONFINITE], tmp_path_factory)


def test_gradients_element_by_element_vs_fp64_fixed_order(tmp_path_factory):
    _judge_all("backward", CHK.BWD_CASES, tmp_path_factory)


def test_gradients_element_by_element_vs_fp64_atomics(tmp_path_factory):
    _judge_all("atomics", CHK.BWD_CASES, tmp_path_factory)
