"""The uncertainty evaluation's definition (INTEGRATION.md "Uncertainty evaluation") on the CPU, through its NumPy
restatement tests/uncert_ref.py, and the tools' new flags.

* with every pixel in a bin of its own, both binned curves equal the textbook stable-sort sparsification of q / 4096 to
  the last bit: the definition means what the literature means, and differs from it only where pixels tie;
* constant log-variance gives a flat curve and AURG = 0; a perfect ranking gives unc == orc and AUSE = 0; a reversed one
  AUSE > 0 and AURG < 0;
* the bin edges and the saturation counts; tiny samples (n = 1, n < steps);
* ``--eval-uncertainty`` / ``--sparsification-steps`` parse, and the flag without ground truth is refused.
"""

from __future__ import annotations

import numpy as np
import pytest

import uncert_ref as U

STEPS = (1, 7, 20, 100)


def tie_free(n=600, seed=3):
    """n pixels, every one in its own u bin and its own o bin, the two orders unrelated (both shuffled)."""
    i = np.arange(n)
    lv = (i / 64.0 - 4.0 + 1.0 / 256.0).astype(np.float32)
    e = (2.0 ** (-7 + i // 256) * (1.0 + (i % 256) / 256.0 + 1.0 / 512.0)).astype(np.float32)
    rng = np.random.default_rng(seed)
    return rng.permutation(lv), rng.permutation(e)


def curves(e, lv, steps):
    row = U.row_from_pixels(e, lv, 1.0, steps)["row"]
    return row[U.HEAD:U.HEAD + steps], row[U.HEAD + steps:], row


@pytest.mark.parametrize("steps", STEPS)
def test_tie_free_curves_equal_the_sorted_sparsification(steps):
    lv, e = tie_free()
    u, o = U.bin_u(lv), U.bin_o(e)
    assert len(set(u.tolist())) == e.size and len(set(o.tolist())) == e.size  # the premise: no two pixels share a bin
    assert 0 < u.min() and u.max() < U.BINS - 1 and 0 < o.min() and o.max() < U.BINS - 1
    q = U.quantise(e)
    assert (q != e.astype(np.float64) * 4096).any()  # q rounds: the curves are of q / 4096, not of e
    unc, orc, row = curves(e, lv, steps)
    assert np.array_equal(unc, U.sparsify_sorted(lv, q / 4096.0, steps))
    assert np.array_equal(orc, U.sparsify_sorted(e, q / 4096.0, steps))
    assert row[0] == e.size and row[1] == q.sum() and row[9] == 0 and row[10] == 0
    assert unc[0] == orc[0] == q.sum() / e.size / 4096.0  # every pixel kept: the mean error


def test_constant_logvar_is_flat():
    _, e = tie_free()
    lv = np.full(e.shape, -1.25, dtype=np.float32)
    unc, orc, row = curves(e, lv, 20)
    assert (np.abs(unc - unc[0]) <= 2 * np.spacing(unc[0])).all()
    assert abs(row[8]) <= 1e-15  # AURG
    assert row[7] > 0 and (np.diff(orc) < 0).all()  # the oracle still falls


def test_perfect_and_reversed_ranking():
    _, e = tie_free()
    e = np.sort(e)
    lv = np.sort(tie_free()[0])
    unc, orc, row = curves(e, lv, 20)  # lv strictly increasing with e
    assert np.array_equal(unc, orc) and row[7] == 0.0 and row[8] > 0
    unc, orc, row = curves(e, lv[::-1].copy(), 20)  # the most certain pixels are the worst
    assert row[7] > 0 and row[8] < 0 and (np.diff(unc) > 0).all()


def test_bin_edges_and_saturation_counts():
    lv = np.array([-40, -32, -32 + 1 / 64, 31.98, 32, 40], dtype=np.float32)
    assert U.bin_u(lv).tolist() == [0, 0, 1, 4094, 4095, 4095]
    e = np.array([0, 2.0 ** -9, 2.0 ** -8, 255.9, 256, 1e6], dtype=np.float32)
    assert U.bin_o(e).tolist() == [0, 0, 0, 4095, 4095, 4095]
    assert U.bin_o(np.array([np.nextafter(np.float32(2.0 ** -8 * (1 + 1 / 256)), np.float32(0)), 2.0 ** -8 * (1 + 1 / 256),
                             1.0, 2.0, 255.0], dtype=np.float32)).tolist() == [0, 1, 2048, 2304, 4094]
    assert U.quantise(e).tolist() == [0, 8, 16, 1048166, 1048576, 2 ** 30]  # 255.9f * 4096 = 1048166.4; 1e6 saturates
    assert U.quantise(np.array([0.5 / 4096, 1.5 / 4096, 2.5 / 4096], np.float32)).tolist() == [0, 2, 2]  # ties to even
    row = U.row_from_pixels(e, lv, 1.0, 4)["row"]
    assert row[0] == 6 and row[9] == 4 and row[10] == 6
    # u bins 0 (two pixels) ... 4095 (two pixels): the all-kept cut is the mean of q
    assert row[U.HEAD] == float(U.quantise(e).sum()) / 6 / 4096.0


@pytest.mark.parametrize("n", [1, 3, 19])
def test_tiny_samples(n):
    lv, e = tie_free()
    steps = 20
    assert min(U.cuts(n, steps)) >= 1 and U.cuts(n, steps)[0] == n
    unc, orc, row = curves(e[:n], lv[:n], steps)
    assert np.isfinite(row).all() and row[0] == n
    q = U.quantise(e[:n])
    assert np.array_equal(unc, U.sparsify_sorted(lv[:n], q / 4096.0, steps))
    assert np.array_equal(orc, U.sparsify_sorted(e[:n], q / 4096.0, steps))
    empty = U.row_from_pixels(e[:0], lv[:0], 1.0, steps)["row"]
    assert empty.shape == (U.HEAD + 2 * steps,) and not empty.any()


def test_zero_error_gives_zero_areas():
    lv, e = tie_free()
    _, _, row = curves(np.zeros_like(e), lv, 20)
    assert row[0] == e.size and row[7] == 0.0 and row[8] == 0.0 and not row[U.HEAD:].any()


def test_coverage_counts_and_nll():
    """e_m = z exp(lv) exactly at lv = 0: covered (<=), and inside the undecided window; lo <= count <= hi."""
    e = np.array([0.25, 0.5, 1.0, 2.0, 3.0, 3.5], dtype=np.float32)
    lv = np.zeros(6, dtype=np.float32)
    r = U.row_from_pixels(e, lv, 1.0, 5)
    assert r["row"][3:7].tolist() == [2, 3, 4, 5]
    assert r["cov_lo"].tolist() == [1, 2, 3, 4] and r["cov_hi"].tolist() == [2, 3, 4, 5]
    assert r["row"][2] == e.astype(np.float64).sum()  # nll_px = e * 1 + 0
    r2 = U.row_from_pixels(e, lv, 2.0, 5)["row"]  # e_m = e / 2
    assert r2[3:7].tolist() == [3, 4, 6, 6] and r2[2] == e.astype(np.float64).sum() / 2


def test_summary_and_aggregate():
    from stereo_depth_estimation_amd import uncert as M

    lv, e = tie_free()
    steps = 7
    rows = np.stack([U.row_from_pixels(e[:400], lv[:400], 1.0, steps)["row"],
                     np.zeros(U.HEAD + 2 * steps), U.row_from_pixels(e[400:], lv[400:], 1.0, steps)["row"]])
    s0, s1, s2 = (M.summary_from_row(r, steps) for r in rows)
    assert s1["valid_pixels"] == 0 and s1["nll"] is None and s1["ause"] is None and s1["sparsification"] is None
    assert s0["nll"] == rows[0, 2] / 400 and s0["ause"] == rows[0, 7] and s0["aurg"] == rows[0, 8]
    assert s0["sparsification"][0] == 1.0 and len(s0["sparsification_oracle"]) == steps
    assert s0["coverage"]["1.0"] == rows[0, 4] / 400 and s0["coverage_nominal"]["1.0"] == 1 - np.exp(-1.0)
    assert s0["saturated_pixels"] == {"logvar": 0, "error": 0}
    agg = M.aggregate_rows(rows, steps)
    assert agg["valid_pixels"] == 600 and agg["samples"] == 2
    assert agg["nll"] == (rows[0, 2] + rows[2, 2]) / 600  # pixel-weighted
    assert agg["ause"] == (s0["ause"] + s2["ause"]) / 2  # the mean over the samples with pixels
    assert agg["sparsification"] == [(a + b) / 2 for a, b in zip(s0["sparsification"], s2["sparsification"])]
    assert M.aggregate_rows(rows[1:2], steps)["nll"] is None
    with pytest.raises(ValueError):
        M.check_steps(0)
    with pytest.raises(ValueError):
        M.check_steps(257)


def test_parsers_take_the_new_flags():
    from stereo_depth_estimation_amd import adapt as A
    from stereo_depth_estimation_amd import predict as P

    a = P.build_parser().parse_args(["--checkpoint", "c.pt", "--dataset-root", "d", "--eval-uncertainty",
                                     "--sparsification-steps", "7"])
    assert a.eval_uncertainty is True and a.sparsification_steps == 7
    a = P.build_parser().parse_args(["--checkpoint", "c.pt", "--dataset-root", "d"])
    assert a.eval_uncertainty is False and a.sparsification_steps is None
    assert P.uncert_options(True, None) == 20 and P.uncert_options(True, 100) == 100 and P.uncert_options() is None
    with pytest.raises(ValueError, match="--dataset-root"):  # no ground truth to evaluate against
        P.main(["--checkpoint", "c.pt", "--left-dir", "l", "--right-dir", "r", "--output-root", "o",
                "--eval-uncertainty"])
    with pytest.raises(ValueError, match="--dataset-root"):
        P.predict_pairs("c.pt", "l", "r", "o", eval_uncertainty=True)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="--sparsification-steps"):
            P.uncert_options(True, bad)
    with pytest.raises(ValueError, match="only with --eval-uncertainty"):
        P.uncert_options(False, 20)

    b = A.build_parser().parse_args(["--checkpoint", "c.pt", "--output-dir", "o", "--dataset-root", "d",
                                     "--eval-uncertainty"])
    assert b.eval_uncertainty is True
    on = A.adapt_options(dataset_root="d", output_dir="o", eval_uncertainty=True)
    assert on["eval_uncertainty"] is True and A.adapt_options(**on) == on
    assert "eval_uncertainty" not in A.adapt_options(dataset_root="d", output_dir="o")  # off: the options as they were
    with pytest.raises(ValueError, match="--dataset-root"):
        A.adapt_options(left_dir="l", right_dir="r", output_dir="o", eval_uncertainty=True)
    with pytest.raises(SystemExit):
        A.main(["--checkpoint", "c.pt", "--output-dir", "o", "--left-dir", "l", "--right-dir", "r", "--eval-uncertainty"])
