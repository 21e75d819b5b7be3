"""The float32 weighted mean of the select kernel's fast path, simulated on the CPU over its whole domain.

wq(sum2, h) = trunc(float32(2 S + 1) x h) with h ~ 0.5 / W must equal S // W for every weight sum W <= 16384 and every
S = q W + r, q <= 100. It is enough to look at r = 0 and r = W - 1 (the value moves monotonically with r between them).
numpy's float32 product is IEEE round-to-nearest, as v_mul_f32 is.

What this shows, and what tests/test_config_space.py can therefore catch on the device:
- with h the float32 nearest to 0.5 / W, or one ulp to either side of it, every mean is right. The general wave kind
  takes h from the hardware reciprocal (documented accuracy 1 ulp; not measured by this suite) followed by one Newton
  step: under that accuracy the step adds margin but is not needed for a right answer, and no input can tell a kernel
  without it apart. Two ulp above is wrong for weight sums near 16384: the margin the step protects is one ulp;
- without the "+ 1" (2 S in place of 2 S + 1) the nearest h is already wrong at residue 0 for thousands of weight sums,
  41, 82 and 122 among them: config_cases.py's NodeResourcesFit vector (20, 21, 41, 40) has these sums, and none of the
  other vectors' sums is affected."""
import numpy as np

F = np.float32
W = np.arange(1, 16385, dtype=np.int64)
H = (F(0.5) / W.astype(F)).astype(F)  # correctly rounded: both operands are exact


def wrong(h, seed=1):
    """Weight sums with some q <= 100 whose mean at residue 0 or W - 1 truncates wrongly."""
    bad = np.zeros(len(W), bool)
    for q in range(101):
        for s in (q * W, q * W + W - 1):
            bad |= ((2 * s + seed).astype(F) * h).astype(F).astype(np.int64) != q
    return W[bad]


def test_mean_is_right_within_one_ulp_of_the_half_reciprocal():
    assert len(wrong(H)) == 0
    assert len(wrong(np.nextafter(H, F(0)))) == 0
    assert len(wrong(np.nextafter(H, F(1)))) == 0


def test_two_ulp_above_is_too_much():
    bad = wrong(np.nextafter(np.nextafter(H, F(1)), F(1)))
    assert len(bad) and bad.min() > 8192


def test_the_seed_is_needed_for_some_weight_sums_only():
    import config_cases as cc
    import weighted_boundary as wb
    bad = set(wrong(H, seed=0).tolist())
    assert {41, 82, 122} <= bad

    def kind_sums(ws):
        return {sum(w for w, c in zip(ws, (True, True, v[4], v[5])) if c) for v in wb.VARIANTS}

    assert kind_sums((20, 21, 41, 40)) == {41, 81, 82, 122}
    for ws in cc.NRF_VECTORS[:-1]:
        assert not kind_sums(ws) & bad, ws
