"""Host logic of the packed text encoder (no GPU): index arrays of a packed batch, prefix-mask detection, alignment,
and the precedence of the config key and the setter.  Everything here runs on host tensors only."""
import types

import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import ops
from mammo_clip_amd.breastclip.model import clip as clipmod
from mammo_clip_amd.breastclip.model.modules import load_text_encoder

TINY = dict(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
            max_position_embeddings=32)


def _fields(pk):
    """the sections of PackedRows.host, as PackedRows.to() cuts them"""
    d, b, r = pk.host, pk.b, pk.rows
    return dict(cu=d[:b + 1], order=d[b + 1:2 * b + 1], eos=d[2 * b + 1:3 * b + 1], row_map=d[3 * b + 1:3 * b + 1 + r],
                pos=d[3 * b + 1 + r:3 * b + 1 + 2 * r], src=d[3 * b + 1 + 2 * r:])


def test_index_arrays_against_a_plain_loop():
    lengths, t0 = [5, 1, 12, 7, 12], 12
    pk = ops.PackedRows(lengths, t0)
    assert pk.t == 16 and pk.b == 5 and pk.max_len == 12 and pk.real == 37      # t: the padded path re-pads T to a multiple of 8
    assert pk.rows == 40 and pk.rows % ops.PackedRows.ALIGN == 0
    f = _fields(pk)
    assert pk.host.dtype == torch.int32 and not pk.host.is_cuda
    assert pk.host.numel() == 3 * pk.b + 1 + 3 * pk.rows
    cu, row_map, pos, src = [0], [], [], []
    for i, n in enumerate(lengths):
        cu.append(cu[-1] + n)
        for k in range(n):
            row_map.append(i * pk.t + k)
            pos.append(k)
            src.append(i * t0 + k)
    pad = pk.rows - pk.real
    assert f["cu"].tolist() == cu
    assert f["eos"].tolist() == [c - 1 for c in cu[1:]]
    assert f["row_map"].tolist() == row_map + [-1] * pad
    assert f["pos"].tolist() == pos + [0] * pad
    assert f["src"].tolist() == src + [0] * pad
    assert f["order"].tolist() == [2, 4, 3, 0, 1]                                # longest first, ties in batch order


def test_alignment_of_the_row_count():
    for lengths in ([1], [8], [9], [3, 4], [256] * 3 + [1], [31, 33]):
        pk = ops.PackedRows(lengths, 256)
        assert pk.rows % 8 == 0 and 0 <= pk.rows - sum(lengths) < 8
        assert (_fields(pk)["row_map"][sum(lengths):] == -1).all()
    try:
        ops.PackedRows([4, 0], 8)
    except ValueError:
        pass
    else:
        raise AssertionError("a zero-length sequence must be rejected")


def test_prefix_mask_detection():
    mask = torch.tensor([[1, 1, 1, 0, 0, 0],        # prefix
                         [1, 1, 1, 1, 1, 1],        # full
                         [1, 0, 1, 0, 0, 0],        # hole
                         [0, 0, 0, 0, 0, 0],        # empty
                         [0, 1, 1, 0, 0, 0],        # does not start at 0
                         [1, 0, 0, 0, 0, 0]])
    ln = ops.prefix_lengths(mask)
    assert not ln.is_cuda and ln.tolist() == [3, 6, 0, 0, 0, 1]
    assert ops.packable([3, 6, 1], 6)
    assert not ops.packable([6, 6], 6)              # all masks full: nothing to skip, the padded launches run
    assert not ops.packable([3, 0, 6], 6)           # one row is no prefix: the whole call falls back
    assert ops.prefix_lengths(mask.bool()).tolist() == [3, 6, 0, 0, 0, 1]


def test_host_masks_give_host_lengths():
    """BreastClip takes the lengths of a HOST attention mask before the tokens move to the device, and only in packed mode"""
    tokens = {"input_ids": torch.ones(2, 4, dtype=torch.long), "attention_mask": torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1]])}
    on = types.SimpleNamespace(text_encoder=types.SimpleNamespace(packed=True))
    off = types.SimpleNamespace(text_encoder=types.SimpleNamespace(packed=False))
    tok = clipmod.BreastClip._tokens_to_device(on, tokens, "cpu")
    assert tok["seq_lengths"].tolist() == [2, 4] and not tok["seq_lengths"].is_cuda
    assert "seq_lengths" not in tokens                                           # the caller's dict is left alone
    tok = clipmod.BreastClip._tokens_to_device(off, tokens, "cpu")
    assert "seq_lengths" not in tok
    assert clipmod._with_host_lengths({"input_ids": tokens["input_ids"]}) is None


def test_config_key_and_setter():
    base = {"source": "huggingface", "name": "x", "pretrained": False, "pooling": "eos", "config": TINY}
    te = load_text_encoder(dict(base), vocab_size=64)
    assert te.packed is False and te.text_encoder.packed is False               # absent = off
    assert load_text_encoder(dict(base, packed=False), vocab_size=64).packed is False
    te = load_text_encoder(dict(base, packed=True), vocab_size=64)
    assert te.packed is True
    assert te.set_packed(False) is te and te.packed is False                     # the setter has the last word
    assert te.text_encoder.set_packed() is te.text_encoder and te.packed is True
    # a call that cannot be packed plans the padded path, on the host, whatever the switch says
    bert = te.text_encoder
    full = torch.ones(2, 8, dtype=torch.long)
    assert bert._packed_plan(full, None, 8, "cpu") is None
    hole = torch.tensor([[1, 0, 1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0]])
    assert bert._packed_plan(hole, None, 8, "cpu") is None
    ragged = torch.tensor([[1, 1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1]])
    pk = bert._packed_plan(ragged, ops.prefix_lengths(ragged), 8, "cpu")
    assert pk.lengths == [3, 8] and pk.rows == 16 and pk.cu.tolist() == [0, 3, 11]
    assert bert.set_packed(False)._packed_plan(ragged, None, 8, "cpu") is None
