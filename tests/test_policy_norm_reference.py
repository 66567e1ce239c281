"""The normaliser's numpy restatement (tests/policy_norm_reference.py) checked without a GPU: against a direct torch float64
transcription of rsl_rl's update over successive batches, and its derived bound against float64 evaluations in three orders
and an math.fsum evaluation, on the cases the GPU test uses."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import policy_norm_reference as R  # noqa: E402

K = 21


def torch_update(x, mean, var, count):
    """rsl_rl's EmpiricalNormalization.update, line by line, in float64"""
    n = x.shape[0]
    count = count + n
    rate = n / count
    var_b, mean_b = torch.var(x, dim=0, unbiased=False, keepdim=True), torch.mean(x, dim=0, keepdim=True)
    delta = mean_b - mean
    mean = mean + rate * delta
    var = var + rate * (var_b - var + delta * (mean_b - mean))
    return mean, var, count


def test_restatement_is_rsl_rls_update_over_successive_batches():
    mean, var, count = R.initial(K)
    tm, tv, tc = torch.zeros(1, K, dtype=torch.float64), torch.ones(1, K, dtype=torch.float64), 0
    for step, n in enumerate((33, 1, R.SEG_ROWS + 33, 17, 600)):
        x = R.seen(R.case_rows(n, K, 40 + step))
        mean, var, count = R.update(x, mean, var, count)
        tm, tv, tc = torch_update(torch.from_numpy(x), tm, tv, tc)
        assert count == tc
        for got, want in ((mean, tm), (var, tv)):
            want = want[0].numpy()
            assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), step
    assert count == 33 + 1 + R.SEG_ROWS + 33 + 17 + 600
    # the affine pair is rsl_rl's (x - mean) / (std + eps), and `until` freezes the state
    a = R.affine32(mean, var)
    x = R.case_rows(5, K, 3)
    want = (x.astype(np.float32).astype(np.float64) - mean) / (np.sqrt(var) + R.EPS)
    got = R.normalise32(x, a).astype(np.float64)
    assert (np.abs(got - want) <= 4 * 2.0 ** -24 * (np.abs(want) + np.abs(mean) / (np.sqrt(var) + R.EPS))).all()
    m2, v2, c2 = R.update(x, mean, var, count, until=count)
    assert c2 == count and np.array_equal(m2, mean) and np.array_equal(v2, var)
    m3, v3, c3 = R.update(x, mean, var, count, until=count + 1)
    assert c3 == count + 5 and not np.array_equal(m3, mean)
    clipped = R.normalise32(x, a, clip=0.5)
    assert np.abs(clipped).max() == np.float32(0.5) and (np.abs(clipped) < 0.5).any()


def one_pass_var(x):
    n = x.shape[0]
    s, ss = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for row in x:
        s, ss = s + row, ss + row * row
    return ss / n - (s / n) ** 2


@pytest.mark.parametrize("n", R.ENVS)
@pytest.mark.parametrize("f32", [False, True])
def test_float64_evaluations_in_three_orders_sit_inside_the_bound(n, f32):
    """three successive updates per case; the exact values against math.fsum; sequential, reversed and segment-wise float64
    inside the bound, element by element; the one-pass variance outside it on the column of mean 1e3 and std 1e-2"""
    state = R.initial(K)
    worst = 0.0
    for step in range(3):
        raw = R.case_rows(n, K, 1000 * n + 10 * step + f32)
        x = R.seen(raw) if f32 else raw
        eb = R.exact_and_bound(x, *state, segments=max(1, (n + 15) // 16))
        # the exact values are what fsum gives: the mean to an ulp, the variance through the centred squares
        for c in range(K):
            m = math.fsum(x[:, c]) / n
            assert abs(eb["mean_b"][c] - m) <= 2 * R.U64 * abs(m)
            v = math.fsum((v - m) ** 2 for v in x[:, c]) / n
            assert abs(eb["var_b"][c] - v) <= eb["b_var_b"][c]
        for order, seg in (("sequential", None), ("reversed", None), ("segments", R.SEG_ROWS), ("segments", 16)):
            mb, vb = R.batch_stats(x, order, seg or R.SEG_ROWS)
            m1, v1, c1 = R.update(x, *state, order=order, seg=seg or R.SEG_ROWS)
            assert c1 == eb["count"]
            for k, got in (("mean_b", mb), ("var_b", vb), ("mean", m1), ("var", v1)):
                ratio = np.abs(got - eb[k]) / eb["b_" + k]
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1.0).all(), (order, seg, k, int(ratio.argmax()), float(ratio.max()))
        assert (eb["var_b"] >= 0).all() and eb["var_b"][1] == 0.0          # the constant column
        if n >= 17:
            assert abs(eb["var_b"][0] - 1e-4) < 1e-4 and eb["b_var_b"][0] < 1e-6 * eb["var_b"][0]
            assert abs(one_pass_var(x)[0] - eb["var_b"][0]) > eb["b_var_b"][0]
        state = R.update(x, *state)
    print(f"n={n} f32={f32}: largest error / bound {worst:.3f}")
