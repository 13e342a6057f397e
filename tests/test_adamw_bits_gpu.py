"""The AdamW step without EMA, held to the bit: mc_adamw_step, mc_adamw_step_clip and mc_adamw_step_ls against digests recorded
on the MI355X before the second-moment form of ``adamw_multi_k`` was pinned and its plumbing moved into csrc/multi_tensor.h
(tests/golden/adamw_bits.json, written by tests/golden/make_golden_adamw_bits.py).  test_ema_gpu.py holds the EMA entry to the
plain one, which cannot see a change that moves both; test_kernels_gpu.py compares with torch within 2e-6.  Cases, inputs and the
digest: tests/_adamw_bits_common.py."""
import json

import pytest

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import lib as L
import _adamw_bits_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(C.GOLDEN) as f:
        return json.load(f)[L.STORAGE]


@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("entry", C.ENTRIES)
def test_plain_adamw_bits_are_the_recorded_ones(golden, entry, layout):
    """two steps of the entry point; every tensor's parameter, exp_avg, exp_avg_sq and image digest equals the recorded one.
    A failure lists the tensors (position:size) and arrays that differ."""
    want, got = golden[f"{entry}/{layout}"], C.run_case(entry, layout)
    assert list(got) == sorted(want) and len(got) == 45
    bad = [(k, a) for k in got for a, x, y in zip(C.ARRAYS, got[k].split(), want[k].split()) if x != y]
    bad += [(k, "arrays") for k in got if len(got[k].split()) != len(want[k].split())]
    assert not bad, (entry, layout, len(bad), bad[:12])
    assert sum(len(v.split()) == 4 for v in got.values()) >= 10           # tensors with an image
