"""The restated launcher of the fp32 dense-layer GEMM (tests/gemm_plan_restatement.py) against the library, and the case table of the
exact sweep (tests/test_gpu_dense_gemm.py) against what it has to cover.  No GPU: npp_gram_fwd_det_scratch_bytes runs the library's
own gemm_prepare on the host and its result holds the number of k ranges."""
import pytest

import npp_amd
import gemm_plan_restatement as R

pytestmark = pytest.mark.skipif(R.fill_overridden(), reason="NPP_GEMM_BATCH_FILL is set: the restated plan holds the default fills")


def test_restated_plan_equals_the_library_s_over_a_gram_sweep():
    """k ranges decoded from npp_gram_fwd_det_scratch_bytes(N, C, hw) = 4 (nb tiles + nb tiles splits 4096 + nb gy splits 64) + 64."""
    L = npp_amd.lib()
    seen = set()
    Cs = [1, 63, 64, 65, 128, 256, 320, 704, 705, 768]            # 704: 11 x 11 = 121 tiles, 705: 12 x 12 = 144 (the 128-tile limit)
    hws = [1, 63, 64, 65, 255, 256, 257, 300, 1000, 2047, 2048, 2049, 2050, 4096, 25600, 65536]
    for N in (1, 2, 3, 6, 40):
        for C in Cs:
            for hw in hws:
                p = R.plan_gram_fwd(N, C, hw, det=True)
                nbytes = int(L.npp_gram_fwd_det_scratch_bytes(N, C, hw))
                assert nbytes == R.det_scratch_bytes(p), (N, C, hw, p)
                assert R.splits_from_det_scratch_bytes(nbytes, N, C) == p.splits, (N, C, hw, p)
                g = (C + 63) // 64
                seen.add(("hw", hw, p.splits > 1))
                seen.add(("tiles<128", g * g < 128, p.splits > 1))
                seen.add(("cap32", p.splits == 32))
                seen.add(("nb>1", N > 1, p.splits > 1))
    for want in [("hw", 255, False), ("hw", 256, True), ("hw", 257, True), ("tiles<128", True, True), ("tiles<128", False, False),
                 ("cap32", True), ("cap32", False), ("nb>1", False, True), ("nb>1", True, True), ("nb>1", True, False)]:
        assert want in seen, f"the sweep never shows {want}"
    assert ("tiles<128", False, True) not in seen and ("hw", 255, True) not in seen


def test_listed_paths_are_the_plans_paths():
    bad = [f"{R.name(c)}: {m}" for c in R.all_cases() for m in [R.path_mismatch(c, R.case_plans(c))] if m]
    assert not bad, "\n".join(bad[:20])


def test_every_sum_of_the_exact_sweep_is_an_integer_below_2_to_24():
    for c in R.all_cases():
        for p in R.case_plans(c):
            assert R.headroom(c, p) < 2 ** 24, (R.name(c), p)


def test_case_table_covers_every_form_load_path_and_split():
    seen = set()
    for c in R.all_cases():
        for p in R.case_plans(c):
            seen.add(("form", p.form, "A", "vec" if p.vec_a else "scalar"))
            seen.add(("form", p.form, "B", "vec" if p.vec_b else "scalar"))
            for why in (p.scalar_a, p.scalar_b):
                if len(why) == 1:                                      # the one reason this operand's loads are scalar
                    seen.add(("scalar because of", why[0]))
            ragged = p.K % p.kchunk != 0
            seen.add(("splits", "1" if p.splits == 1 else ("32" if p.splits == 32 else ("ragged" if ragged else "even"))))
            if p.splits > 1 and p.K >= 256:
                seen.add(("K split", p.K))
            seen.add(("K", p.K))
            seen.add(("M", p.M))
            seen.add(("N", p.N))
            seen.add(("nb>1", p.nb > 1, "split" if p.splits > 1 else "one range"))
            seen.add(("mode", p.mode))
    want = [("form", f, o, l) for f in ("KC/KC", "KC/NC", "MC/KC", "MC/NC") for o in "AB" for l in ("vec", "scalar")]
    want += [("scalar because of", w) for w in ("pointer", "extent", "ld", "batch")]
    want += [("splits", s) for s in ("1", "ragged", "32")]
    want += [("K", k) for k in (255, 256, 257)] + [("K split", 256), ("K split", 257)]
    want += [(d, v) for d in "MN" for v in (1, 63, 64, 65)]
    want += [("nb>1", True, "split"), ("nb>1", True, "one range"), ("nb>1", False, "split"), ("mode", "atomic"), ("mode", "two_pass")]
    missing = [w for w in want if w not in seen]
    assert not missing, f"the case table does not reach: {missing}"
