"""The e4m3 reference of tests/_fp8_ref.py, without a device: on all 65 536 bf16 and all 65 536 f16 bit patterns and each amax
of the quantiser tests, `rne_code` equals torch's CPU float8_e4m3fn cast of the clamped fp32 value, byte for byte -- two
independent roundings (a table search in fp64 here, bit manipulation there).  The same sweep proves the conditions that keep
tests/test_fp8_exact_gpu.py honest: how many of its inputs saturate, land in the e4m3 subnormal range and sit exactly on a
rounding tie, so a changed amax list fails here instead of silently emptying the GPU test.

Counts (fp64, exact).  Saturated and subnormal-range inputs number in the thousands for every amax at bf16 storage.  Ties are
a number-theoretic matter: a tie has at most 5 significant bits, the scaled value is fl32(x * scale) with an 8-bit (bf16) or
11-bit (f16) x, so with a power-of-two scale (amax 448, 57344) every binade of the e4m3 range holds 8 ties per sign (252 in
all), while a scale with a wide significand leaves only the x whose product happens to be that short: 32 for amax 1, 3 and
2^-20 and 2 for amax 0.37109375 at bf16.  The bound of 100 therefore holds per amax for the power-of-two scales and for the
sweep as a whole; the power-of-two scales have ties of both parities (down to an even code, up to an even code).  f16 storage cannot saturate a thousand inputs under amax
57344 (its largest value is 65504) nor reach the subnormal range under amax 2^-20 (its smallest is 2^-24, scaled to 28);
there the counts are asserted where the format allows them.
"""
import pytest
import torch

import _fp8_ref as R

DTYPES = [torch.bfloat16, torch.float16]
POW2 = (448.0, 57344.0)                  # amax values whose scale is a power of two


def _a32(amax):
    return torch.tensor(amax, dtype=torch.float32)


def _torch_code(v):
    """torch's own conversion of the clamped value (NaN stays NaN = 0x7f / 0xff)"""
    return torch.where(torch.isnan(v), v, v.clamp(-R.MAX, R.MAX)).to(torch.float8_e4m3fn).view(torch.uint8)


def test_table_is_e4m3():
    """the table against the format's definition, code by code, and against torch's decoding of the same bytes"""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    mine, theirs = R.decode(codes), codes.view(torch.float8_e4m3fn).to(torch.float64)
    assert torch.equal(torch.isnan(mine), torch.isnan(theirs)) and int(torch.isnan(mine).sum()) == 2
    ok = ~torch.isnan(mine)
    assert torch.equal(mine[ok], theirs[ok])
    assert torch.equal(torch.signbit(mine[ok]), torch.signbit(theirs[ok]))          # 0x80 decodes to -0.0
    assert torch.equal(R.rne_code(mine), codes)                                     # every code is its own rounding
    assert float(R.decode(torch.tensor([0x38], dtype=torch.uint8))) == 1.0 and float(R.decode(torch.tensor([0x4e], dtype=torch.uint8))) == 7.0
    assert float(R.decode(torch.tensor([0xb8], dtype=torch.uint8))) == -1.0


@pytest.mark.parametrize("amax", R.AMAXES, ids=lambda a: f"amax_{a:g}")
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_rne_code_equals_torch_on_every_input(dtype, amax):
    x = R.all_patterns(dtype)
    v = R.scaled(x, _a32(amax))
    got, want = R.quant_ref(x, _a32(amax)), _torch_code(v)
    nan = torch.isnan(x)
    assert int(nan.sum()) > 0 and bool((got[nan] % 128 == R.NAN_CODE).all()) and bool((want[nan] % 128 == R.NAN_CODE).all())
    bad = (got != want) & ~nan
    assert int(bad.sum()) == 0, f"{int(bad.sum())} mismatches, first x bits {int(x.view(torch.int16)[bad][0]) & 0xffff:#06x}"
    # the conditions of the GPU test, counted exactly
    fin = ~torch.isnan(v)
    a = v[fin].double().abs()
    sat = int((a >= R.MAX).sum())
    sub = int(((a > 0) & (a < 2.0 ** -6)).sum())
    tie = R.is_tie(v)
    ties = int(tie.sum())
    print(f"{dtype} amax {amax:g}: {sat} saturated, {sub} in the subnormal range, {ties} ties")
    if dtype == torch.bfloat16:
        assert sat >= 1000 and sub >= 1000, (sat, sub)
        # 16-bit denormal inputs quantise to +-0 under every amax of the list: flushing them cannot change a code
        den = (x.view(torch.int16) & 0x7f80) == 0
        assert int(den.sum()) == 256 and bool((got[den] % 128 == 0).all())
    else:
        assert sat >= (1000 if amax != 57344.0 else 514) and (sub >= 400 or amax == 2.0 ** -20), (sat, sub)
    assert ties >= (100 if amax in POW2 else 2), ties
    # both parities: a tie that goes down to an even code and one that goes up to an even code
    _, lo, _ = R.neighbours(v[tie])
    assert amax not in POW2 or (bool((lo % 2 == 0).any()) and bool((lo % 2 == 1).any()))
    assert bool((got[tie] % 2 == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_the_sweep_as_a_whole_has_hundreds_of_ties(dtype):
    x = R.all_patterns(dtype)
    n = sum(int(R.is_tie(R.scaled(x, _a32(amax))).sum()) for amax in R.AMAXES)
    assert n >= 500, n


def test_permuted_order_is_a_permutation():
    x = R.all_patterns(torch.bfloat16, seed=5).view(torch.int16).to(torch.int32) & 0xffff
    assert sorted(x.tolist()) == list(range(65536)) and x[:64].tolist() != list(range(64))


def test_scale_rules():
    """amax 0 -> scale 1; NaN amax -> NaN; a tiny amax keeps the scale finite, so zeros stay zeros, +-amax gives +-448 and
    amax / 2 gives 224; above the threshold the pre-factor is 1 and the arithmetic is the plain x * (448 / amax)"""
    assert float(R.scale_of(_a32(0.0))) == 1.0
    assert bool(torch.isnan(R.scale_of(_a32(float("nan")))))
    tiny = _a32(2.0 ** -125)
    assert float(torch.tensor(448.0) / tiny) == float("inf") and float(R.scale_of(tiny)) == 448.0 * 2.0 ** 61
    x = torch.tensor([0.0, -0.0, 2.0 ** -125, -2.0 ** -125, 2.0 ** -126, -2.0 ** -126], dtype=torch.bfloat16)
    assert R.quant_ref(x, tiny).tolist() == [0x00, 0x80, 0x7e, 0xfe, 0x76, 0xf6]
    for amax in R.AMAXES + (2.0 ** -100,):
        assert float(R.pre_of(_a32(amax))) == 1.0
    for amax in (2.0 ** -101, 2.0 ** -126, 2.0 ** -149):                            # down to the smallest fp32 denormal
        assert float(R.pre_of(_a32(amax))) == R.PRE and bool(torch.isfinite(R.scale_of(_a32(amax))))
        assert R.quant_ref(torch.zeros(2, dtype=torch.bfloat16), _a32(amax)).tolist() == [0, 0]
    assert bool((R.quant_ref(R.all_patterns(torch.bfloat16), _a32(float("nan"))) % 128 == R.NAN_CODE).all())
    inf = torch.tensor([float("inf"), -float("inf")], dtype=torch.bfloat16)
    assert R.quant_ref(inf, _a32(1.0)).tolist() == [0x7e, 0xfe]                     # Inf saturates under a finite amax
    assert bool((R.quant_ref(inf, _a32(float("inf"))) % 128 == R.NAN_CODE).all())   # measured amax Inf: scale 0, Inf * 0 = NaN
