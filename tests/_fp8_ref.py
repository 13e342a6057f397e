"""OCP e4m3 ("float8_e4m3fn": no infinities, one NaN per sign) from first principles, in plain torch -- the reference of
tests/test_fp8_exact.py (CPU: checked against torch's own cast on every 16-bit input) and tests/test_fp8_exact_gpu.py (the
quantiser of csrc/fp8.hip, byte for byte).

Code c = s eeee mmm.  e = 0: m * 2^-9 (subnormal); e > 0: (1 + m / 8) * 2^(e - 7); 0x7e = 448 is the largest finite value and
0x7f / 0xff are NaN.  The 127 non-negative finite values are strictly increasing in their code, so rounding to nearest is a
search in a sorted table and "ties to even" is "ties to the even code".  Every table entry and every fp32 input is exact in
fp64, so the two distances compared below are exact and a tie is recognised as one.

Functions work on the device of their argument.
"""
import torch

F64 = torch.float64
MAX = 448.0
FLT_MAX = 3.4028234663852886e38
NAN_CODE = 0x7f

TABLE = torch.tensor([m * 2.0 ** -9 for m in range(8)] + [(1 + m / 8) * 2.0 ** (e - 7) for e in range(1, 16) for m in range(8)],
                     dtype=F64)[:127]
assert TABLE.numel() == 127 and float(TABLE[-1]) == MAX and float(TABLE[1]) == 2.0 ** -9 and float(TABLE[8]) == 2.0 ** -6
assert bool((TABLE[1:] > TABLE[:-1]).all())

# the amax values of the exhaustive quantiser tests: a unit scale, a power-of-two scale (57344 = 448 * 2^7), three scales
# with a full fp32 significand (448, 448 / 3, 448 / 0.37109375) and a large one (448 * 2^20)
AMAXES = (448.0, 1.0, 3.0, 0.37109375, 57344.0, 2.0 ** -20)


def neighbours(v):
    """|v| (fp64, NaN -> 0) with the table entries below and above it: (a, lo, hi) with TABLE[lo] <= a <= TABLE[hi],
    lo == hi exactly when a is a table entry or lies outside the table's range"""
    a = torch.nan_to_num(v.to(F64).abs(), nan=0.0).clamp(max=MAX)
    tab = TABLE.to(a.device)
    idx = torch.searchsorted(tab, a)                    # first entry >= a
    hi = idx.clamp(max=126)
    lo = torch.where(tab[hi] == a, hi, (idx - 1).clamp(min=0))
    return a, lo, hi


def is_tie(v):
    """v lies exactly half way between two neighbouring e4m3 values (decided in fp64, exactly)"""
    a, lo, hi = neighbours(v)
    tab = TABLE.to(a.device)
    return (lo != hi) & (a - tab[lo] == tab[hi] - a) & ~torch.isnan(v)


def rne_code(v):
    """e4m3 code (uint8) of a float tensor, round to nearest, ties to the even code; |v| beyond 448 saturates; the sign
    bit is v's own (signbit: -0.0 and negatives that round to zero give 0x80); NaN gives 0x7f / 0xff"""
    a, lo, hi = neighbours(v)
    tab = TABLE.to(a.device)
    dlo, dhi = a - tab[lo], tab[hi] - a
    even_lo = lo % 2 == 0
    code = torch.where((dlo < dhi) | ((dlo == dhi) & even_lo), lo, hi)
    code = torch.where(torch.isnan(v), torch.full_like(code, NAN_CODE), code)
    return (code + 128 * torch.signbit(v).to(code.dtype)).to(torch.uint8)


def decode(code):
    """uint8 e4m3 codes -> fp64 values (NaN for 0x7f / 0xff)"""
    c = code.to(torch.int64)
    tab = torch.cat([TABLE, torch.tensor([float("nan")], dtype=F64)]).to(code.device)
    return torch.where(c >= 128, -tab[c % 128], tab[c % 128])


TINY_AMAX, PRE = 2.0 ** -100, 2.0 ** 64


def pre_of(amax32):
    """the power of two that amax and x are multiplied by before the division: 2^64 for 0 < amax < 2^-100, else 1.  It keeps
    the scale finite for every positive finite amax (448 / amax overflows below 448 / FLT_MAX ~ 1.3e-36, and 0 * inf = NaN)
    and, being a power of two, changes no rounding: the result is what fp32 with an unbounded exponent would give"""
    amax32 = amax32.to(torch.float32)
    return torch.where((amax32 > 0) & (amax32 < TINY_AMAX), torch.full_like(amax32, PRE), torch.ones_like(amax32))


def scale_of(amax32):
    """the quantiser's scale, in fp32 like the kernel: 448 / (amax * pre); 1 for amax == 0; NaN for a NaN amax"""
    amax32 = amax32.to(torch.float32)
    s = torch.tensor(MAX, dtype=torch.float32, device=amax32.device) / (amax32 * pre_of(amax32))
    return torch.where(amax32 > 0, s, torch.where(torch.isnan(amax32), amax32, torch.ones_like(amax32)))


def scaled(x16, amax32):
    """(float(x) * pre) * scale in fp32, before the clamp"""
    return (x16.to(torch.float32) * pre_of(amax32)) * scale_of(amax32)


def quant_ref(x16, amax32):
    """mc_quant_fp8_bf16's documented arithmetic: v = float(x) * scale in fp32, finite v clamped to +-448, rounded to the
    nearest e4m3 value (ties to even); NaN (a NaN input, a NaN amax, Inf * 0) gives a NaN code"""
    v = scaled(x16, amax32)
    return rne_code(torch.where(torch.isnan(v), v, v.clamp(-MAX, MAX)))


def all_patterns(dtype, seed=None):
    """the 65 536 values of a 16-bit float type, in code order or (seed) in a seeded permuted order"""
    bits = torch.arange(65536, dtype=torch.int32)
    if seed is not None:
        bits = bits[torch.randperm(65536, generator=torch.Generator(device="cpu").manual_seed(seed))]
    return bits.to(torch.int16).view(dtype)
