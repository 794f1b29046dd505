"""CPU (no GPU): the conditions tests/test_gpu_exact.py rests on, checked on the fp64 reference alone, so that a bad seed,
amplitude or case fails here and not on the device.

  * rne_bf16 is round-to-nearest-even (against bit arithmetic, with exact ties in both directions);
  * every case of the exact regime has a reference that is on the bf16 grid throughout (inputs, output, padded-domain
    gradient, dx with and without `add`) and integer weight gradients below 2^24: every rounding is the identity there;
  * every case of the rounding regime leaves the bf16 grid on >= 20 % of each bf16 output tensor, >= 1 % of all of them are
    exact ties, and no case runs on Winograd;
  * the rounding model of a backward-data form follows from its kernel name, and where it says "two" the two models differ on
    the case's reference (the choice is observable);
  * a tanh case keeps its kernels when it runs with act = "none";
  * the ReLU norms of part d leave at most 1 % of their elements near the kink."""
import pytest
import torch

from tests import lattice as L


@pytest.fixture(scope="module")
def lib():
    from munit_amd import _lib
    return _lib.load()


def _rne_bits(t):
    """Hand-written round-to-nearest-even of fp32 bit patterns to their upper 16 bits (finite values)."""
    bits = t.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    bits = bits + 0x7FFF + ((bits >> 16) & 1)
    return (bits >> 16) & 0xFFFF


def test_rne_bf16_is_round_to_nearest_even():
    pinned = {257.0: 256.0, 259.0: 260.0, -257.0: -256.0, -259.0: -260.0, 514.0: 512.0, 518.0: 520.0, 1028.0: 1024.0,
              1036.0: 1040.0, -1028.0: -1024.0, -1036.0: -1040.0, 256.0: 256.0, 512.0: 512.0, 1024.0: 1024.0, 255.0: 255.0,
              258.0: 258.0, 0.5: 0.5, 128.5: 128.0, 129.5: 130.0, -128.5: -128.0, 257.5: 258.0, 256.99: 256.0, 257.01: 258.0}
    t = torch.tensor(list(pinned), dtype=torch.float64)
    assert L.rne_bf16(t).double().tolist() == list(pinned.values())
    assert L.is_tie(t).tolist() == [abs(v) in (257, 259, 514, 518, 1028, 1036, 128.5, 129.5) for v in pinned]
    g = torch.Generator().manual_seed(1)
    ints = torch.arange(-4200, 4201, dtype=torch.float64)
    many = torch.cat([t, ints, ints / 2, torch.randn(20000, generator=g, dtype=torch.float64) * 300])
    got = L.rne_bf16(many).view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(got, _rne_bits(many))
    assert bool(L.exactly_bf16(torch.tensor([256.0, 258.0, 1024.0, 1032.0, 4096.0 - 16])).all())
    assert not bool(L.exactly_bf16(torch.tensor([257.0, 1028.0, 4096.0 - 8])).any())
    assert L.ulp_bf16(torch.tensor([1.0, 255.0, 256.0, 300.0, -1024.0, 0.75])).tolist() == [2.0 ** -7, 1.0, 2.0, 2.0, 8.0, 2.0 ** -8]


def test_lattice_draws_the_stated_sets():
    x = L.lattice((4, 64, 9, 7), 1, (-1, 0, 1), 0.25)
    assert x.dtype == torch.float64 and set(x.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert abs(float((x != 0).double().mean()) - 0.25) < 0.02
    w = 4 * L.lattice((64, 64, 3, 3), 2, (-1, 0, 1))
    assert set(w.unique().tolist()) == {-4.0, 0.0, 4.0} and abs(float((w != 0).double().mean()) - 2 / 3) < 0.02
    assert torch.equal(L.lattice((5, 5), 3, range(-4, 5)), L.lattice((5, 5), 3, range(-4, 5)))


def test_the_case_lists_are_the_suites():
    from tests import test_gpu_bf16 as B16, test_gpu_bf16s as B16S, test_gpu_f32x3 as X3, test_gpu_ops as T
    cases = L.exact_cases()
    assert len(cases) == len(set(cases))
    have = {(c, m) for c, m, _, _ in cases}
    assert {(tuple(c), "f32") for c in T.CONV_CASES} <= have and {(tuple(c), "f32x3") for c in X3.F32X3_CASES} <= have
    assert {(tuple(c), "bf16") for c in B16.CASES} <= have
    assert {(c[:7] + ("none",) + c[7:], "bf16") for c in B16.WGRAD_CASES} <= have
    assert {((k, n, 1, 1, 0, "zero", 0, a, b, 1, 1), "f32") for b, k, n, a in T.LINEAR_CASES} <= have
    assert len([c for c in cases if c[1] == "bf16s"]) == len(B16S.CASES) == len(L.rounding_cases())
    assert len(L.LEFT_OUT) <= 2


@pytest.mark.parametrize("entry", L.exact_cases(), ids=L.case_id)
def test_exact_regime_reference_stays_on_the_bf16_grid(entry):
    case = entry[0]
    inp = L.exact_inputs(entry)
    ref = L.conv_reference(case, inp["x"], inp["w"], inp["b"], inp["dy"], act="none" if case[7] == "tanh" else None)
    cond = L.exact_regime_conditions(entry, inp, ref)
    assert all(cond.values()), cond
    # the outputs are not trivially zero: a dropped tap must be able to show
    share = {n: float((ref[n] != 0).double().mean()) for n in ("pre", "dx", "dw")}
    assert share["pre"] > 0.5 and share["dx"] > 0.1 and share["dw"] > 0.02, share


def test_rounding_regime_leaves_the_grid_and_hits_ties(lib):
    total = ties = 0
    for entry in L.rounding_cases():
        case, compute, din, dout = entry
        names = L.kernel_names(lib, entry, "none")
        assert not any("wino" in n for n in names), (entry, names)
        inp = L.rounding_inputs(entry)
        assert all(bool(L.exactly_bf16(inp[n]).all()) for n in ("x", "w", "dy", "add")), entry
        ref = L.conv_reference(case, inp["x"], inp["w"], inp["b"], inp["dy"], act="none")
        assert L.integers_below_2_24(ref["dw"]) and L.integers_below_2_24(ref["db"])
        for name, t, dt in (("y", ref["pre"], dout), ("dx", ref["dx"], din)):
            if dt != L.BF:
                continue
            inexact = 1 - float(L.exactly_bf16(t).double().mean())
            assert inexact >= 0.2, (entry, name, inexact)
            total += t.numel()
            ties += int(L.is_tie(t).sum())
        model = L.dgrad_rounding_model(names[1], din == L.BF, False)
        if model == "two":      # observable: the two models give different bits on this very reference
            assert not torch.equal(L.two_rounding(ref), L.one_rounding(ref["dx"])), entry
    assert ties >= 0.01 * total, (ties, total)


def test_rounding_model_follows_the_kernel_name(lib):
    two, one = set(), set()
    for entry in L.rounding_cases():
        name = L.kernel_names(lib, entry, "none")[1]
        (two if L.dgrad_rounding_model(name, entry[2] == L.BF, False) == "two" else one).add((name, entry[2] == L.BF))
    assert all("fold_kernel<bf16_t>" in n and bf for n, bf in two) and len(two) >= 3, two
    assert not any("fold_kernel<bf16_t>" in n for n, _ in one), one
    # the strided, up-sampling and image-head layers fold a bf16 buffer; the LDS patch and the 1x1 layers write dx once
    assert {n for n, bf in one if bf} == {"conv_igemm_kernel<128, true, 2, 4> (LDS-patch fold)", "conv_igemm_kernel<64, true, 2, 4> (LDS-patch fold)",
                                        "conv_igemm_kernel<64, true, 1, 4> direct", "conv_igemm_kernel<128, true, 1, 4> direct"}, one
    assert L.dgrad_rounding_model("conv_igemm_kernel<64, true, 1, 4> direct", True, True) == "two"
    assert L.dgrad_rounding_model("conv_igemm_kernel<64, true, 1, 4> phases + fold_kernel<bf16_t>", False, True) == "one"
    assert not L.dgrad_takes_add("conv_igemm_kernel<64, true, 2, 4> (LDS-patch fold)", True)
    assert L.dgrad_takes_add("conv_igemm_kernel<.., 2, 3> (LDS-patch fold)", False)


def test_tanh_cases_run_the_same_kernels_without_the_activation(lib):
    tanh = [e for e in L.exact_cases() if e[0][7] == "tanh"]
    assert len(tanh) >= 3
    for entry in tanh:
        assert L.kernel_names(lib, entry) == L.kernel_names(lib, entry, "none"), entry


def test_no_exact_case_is_refused(lib):
    for entry in L.exact_cases() + L.HEAD_CASES:
        names = L.kernel_names(lib, entry, "none" if entry[0][7] == "tanh" else None)
        assert not any(n.startswith("refused") or n == "invalid" for n in names), (entry, names)


@pytest.mark.parametrize("shape", L.NORM_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("kind", [k for k in L.NORM_KINDS if k.endswith("relu")])
def test_norm_inputs_leave_few_elements_near_the_kink(kind, shape):
    d = L.norm_inputs(kind, shape)
    pre = L.norm_pre(kind, d, d)
    share = float(L.near_kink(pre, L.FWD_TOL).double().mean())
    assert share <= 0.01, share
