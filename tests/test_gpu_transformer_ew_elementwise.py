"""Every kernel of csrc/transformer_ew.hip, element by element against fp64.

tests/test_gpu_transformer.py judges these kernels by one number per tensor, max|got - ref| / max|ref| < 1e-2 against torch's fp32 on
one Gaussian input per shape: a variance divided by D - 1, a one-pass variance, a residual added after the bf16 rounding, a truncated
store, a lane's last vector left out of the statistics, one block's rows missing from dgamma or a skipped GELU tail element all pass it.
Here tests/helpers/transformer_ew_check.py runs tanh-GELU forward / backward (bf16 and fp32: tail-only sizes, the first size whose
grid-stride loop iterates twice, and a sweep of all 65 280 finite bf16 bit patterns), ``mas_gelu_tanh_bwd_colsum`` (grid units 1, 3,
257, idle threads, threads that loop), LayerNorm forward (four dtype pairs, with and without residual, D from one vector to the
envelope's maximum, more rows than waves), LayerNorm backward ({2, 3 partial rows} x {dx_add absent, present}, 201 and >= 768 blocks
through ``fold_rows_kernel``), the LayerNorm pair and ``mas_colsum`` (1 ... 128 slices), records every output -- ``mean_rstd`` and the
column sums handed to ``_ColsumHint`` included -- with ``ops.last_kernel()`` after each launch, and judges on the CPU: each stage on its
own arithmetic (the backward is fed the reference's mean_rstd; y2 of the pair is judged against the fp64 LayerNorm of the kernel's own
xnew; dx_colsum against the fp64 column sum of the kernel's own dx), every bound derived in the helper's docstring.

  * gauss: rows rotate through (mu, sigma) = (0.3, 1.5), (8, 1), (-20, 0.5) (+ (300, 0.05) for fp32 inputs), one constant row and one
    row with a 100-sigma outlier per tensor; EVERY element of y, mean, rstd, xnew, y2, both pairs of statistics, dx, dgamma, dbeta and
    dx_colsum must be inside its bound, the constant row must give fl(beta + res) bitwise, and two runs of every reduction must be
    bitwise equal;
  * exact: eps = 0, x = 2^(row % 5 - 2) s(col): mean and rstd bitwise, y / xnew / y2 / dgamma / dbeta (and dx for D a power of two)
    bitwise the correctly rounded exact value, with at least 5 % exact bf16 ties among the bf16 outputs; integer column sums bitwise.

REQUIRED (in the helper) lists the (launch, feature) pairs each family has to reach; a dispatch change that leaves a case vacuous fails.

Measured on an MI355X (256 CUs): the worst K any element needed (|error| less the store's own rounding, over 2^-23 x the bound's
magnitude term), the K chosen by the rule "worst seen, doubled, next power of two", and the worst |error| / bound with it:
  GELU y       tanhf (fp32) K needed 0.997 -> 2;  __expf (bf16) 0.483 -> 1
  GELU dx      tanhf 5.08 -> 16;  __expf 15.7 -> 32 (the absolute error of t times 0.5 |x| k (1 + 3 c x^2), ~10 at |x| = 5)
  LN mean      1.31 -> 4      LN rstd  0.797 -> 2      LN y  1.43 -> 4 (forward 1.43, xnew 1.28, y2 1.25)      LN dx  1.57 -> 4
  sums         dgamma 1.70, dbeta 1.14, dx_colsum 1.28 (LayerNorm) / 1.64 (GELU fp32), mas_colsum 1.21 -> 4
Worst |error| / bound per family with these K (1 = the bound), gauss mode and the sweep:
  GELU         y bf16 0.996, fp32 0.499;  dx bf16 0.995, fp32 0.317
  LN forward   (bf16->bf16, bf16->fp32, fp32->bf16, fp32->fp32)  mean 0.121 / 0.113 / 0.280 / 0.275,  rstd 0.356 / 0.344 / 0.367 / 0.328,
               y 0.995 / 0.265 / 0.993 / 0.357
  LN backward  (bf16<-bf16, bf16<-fp32, fp32<-bf16, fp32<-fp32)  dx 0.996 / 0.996 / 0.391 / 0.376,  dgamma 0.426 / 0.398 / 0.348 / 0.335,
               dbeta 0.069 / 0.235 / 0.021 / 0.285,  dx_colsum 0.228 / 0.168 / 0.321 / 0.315
  LN pair      xnew mean / rstd / value: bf16 0.113 / 0.345 / 0.286, fp32 0.328 / 0.279 / 0.320;  y2 (against the kernel's own xnew):
               bf16 0.231 / 0.391 / 0.995, fp32 0.262 / 0.399 / 0.312
  column sums  gelu_bwd_colsum bf16 0.142, fp32 0.410;  mas_colsum bf16 0.161, fp32 0.303
  The bf16 value figures sit just under 1 because their bound is the rounding itself (a near-tie at 0.99 of half an ulp); what the fp32
  arithmetic adds shows in the fp32 tensors, the statistics and the sums.  exact mode: every equality holds (mean, rstd, y, xnew, y2,
  dgamma, dbeta, dx at D a power of two, the integer column sums, the constant rows); every rerun of a reduction is bitwise equal.
Findings.  ``gelu_bwd_kernel`` returned NaN for every |x| >= 2^64 (a * a overflows, (1 - t^2) * inf): 49 152 of the 65 280 x 3 sweep
outputs in bf16 and as many in fp32; the kernel now yields the limit there (dy or 0), and the sweep run on the build before and the
build after differs bitwise in exactly those 49 152 outputs per dtype and in no other.  ``mas_colsum`` lacked ``MAS_ENTER()``.  No
other element was outside a bound; no bf16 bound needs more than the one store rounding.  At the longest row count of the backward the
two widest D run in gauss mode alone (``ln_bwd_cases``).  The five tests take ~7 s together, the backward 5 s of them."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import transformer_ew_check as CHK  # noqa: E402

SWITCHES = ("MAS_LN_FWD_BLOCKS_PER_CU", "MAS_LN_PAIR_FWD_BLOCKS_PER_CU", "MAS_GELU_COLSUM", "MAS_LN_PAIR")


def _judge_all(part):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert not [k for k in SWITCHES if k in os.environ], "the launch geometry restated in the helper is the default one: unset " + ", ".join(SWITCHES)
    from mas_hip import ops
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    failures, worst, kneed = CHK.judge_family(part, cus, lambda c, mode, ins: CHK.run_case(c, mode, ins, ops, dev))
    torch.cuda.synchronize()
    print(f"worst |error| / bound and K needed per family, {part}, {cus} CUs:")
    for fam in sorted(worst):
        print(f"  {fam:52s} {worst[fam]:.3f}   {kneed[fam]:.3f}")
    assert not failures, "\n".join(failures[:60])


def test_gelu_element_by_element_vs_fp64():
    _judge_all("gelu")


def test_layernorm_forward_element_by_element_vs_fp64():
    _judge_all("ln_fwd")


def test_layernorm_backward_element_by_element_vs_fp64():
    _judge_all("ln_bwd")


def test_layernorm_pair_element_by_element_vs_fp64():
    _judge_all("pair")


def test_column_sums_element_by_element_vs_fp64():
    _judge_all("colsum")
