"""distributed.pack_records on matches that already are a record: mk1 / mk2 / scores as views of one contiguous
(B, Mx, 6) float32 tensor and the validity mask tagged with it (what ops.mnn_from_duals[_dots] return) come back as that
tensor itself; anything else -- and anything edited since the tag -- is concatenated as before, with the same values."""
import torch

from onnx_image_processing_amd import distributed as D


def _slow(mk1, mk2, scores, valid):
    """The concatenation, written out independently of pack_records."""
    out = torch.empty(tuple(scores.shape) + (6,), dtype=torch.float32)
    out[..., 0:2], out[..., 2:4], out[..., 4], out[..., 5] = mk1, mk2, scores, valid.to(torch.float32)
    return out


def _record(seed=0, b=3, mx=7):
    g = torch.Generator().manual_seed(seed)
    rec = torch.rand((b, mx, 6), generator=g)
    valid = torch.rand((b, mx), generator=g) > 0.5
    rec[..., 5] = valid.to(torch.float32)
    return rec, valid


def _views(rec):
    return rec[..., 0:2], rec[..., 2:4], rec[..., 4]


def _falls_back(mk1, mk2, scores, valid, rec):
    want = _slow(mk1, mk2, scores, valid)
    got = D.pack_records(mk1, mk2, scores, valid)
    assert got.data_ptr() != rec.data_ptr()
    assert got.is_contiguous() and got.dtype == torch.float32
    assert torch.equal(got, want)


def test_tagged_views_return_the_base():
    rec, valid = _record()
    D.tag_record(rec, valid)
    mk1, mk2, scores = _views(rec)
    got = D.pack_records(mk1, mk2, scores, valid)
    assert got is rec and got.data_ptr() == rec.data_ptr()
    assert torch.equal(got, _slow(mk1, mk2, scores, valid))
    a, b, c, d = D.unpack_records(got)
    assert torch.equal(a, mk1) and torch.equal(b, mk2) and torch.equal(c, scores) and torch.equal(d, valid)
    assert D.pack_records(mk1, mk2, scores, valid) is rec          # and again: asking changes nothing


def test_one_pair_and_one_slot():
    for b, mx in ((1, 5), (4, 1), (1, 1)):
        rec, valid = _record(1, b, mx)
        D.tag_record(rec, valid)
        assert D.pack_records(*_views(rec), valid) is rec


def test_cloned_member_falls_back():
    rec, valid = _record(2)
    D.tag_record(rec, valid)
    mk1, mk2, scores = _views(rec)
    _falls_back(mk1.clone(), mk2, scores, valid, rec)
    _falls_back(mk1, mk2.clone(), scores, valid, rec)
    _falls_back(mk1, mk2, scores.clone(), valid, rec)
    _falls_back(mk1, mk2, scores, valid.clone(), rec)              # the copy of a tagged mask carries no tag


def test_member_from_another_base_falls_back():
    rec, valid = _record(3)
    other, _ = _record(4)
    D.tag_record(rec, valid)
    mk1, mk2, scores = _views(rec)
    _falls_back(other[..., 0:2], mk2, scores, valid, rec)
    _falls_back(mk1, mk2, other[..., 4], valid, rec)
    other_valid = _record(5)[1]
    D.tag_record(other, other_valid)                                # a mask tagged, but with another record
    _falls_back(mk1, mk2, scores, other_valid, rec)


def test_wrong_offsets_fall_back():
    rec, valid = _record(6)
    D.tag_record(rec, valid)
    mk1, mk2, scores = _views(rec)
    _falls_back(mk2, mk1, scores, valid, rec)                       # swapped
    _falls_back(rec[..., 1:3], mk2, scores, valid, rec)
    _falls_back(mk1, mk2, rec[..., 3], valid, rec)
    _falls_back(mk1, mk2, rec[..., 5], valid, rec)
    _falls_back(mk1[:2], mk2[:2], scores[:2], valid[:2], rec)       # fewer pairs than the base holds


def test_non_contiguous_base_falls_back():
    store = torch.rand((3, 7, 12))
    rec = store[..., ::2]                                           # (3, 7, 6), strides (84, 12, 2)
    valid = rec[..., 5] > 0.5
    D.tag_record(rec, valid)
    _falls_back(*_views(rec), valid, rec)
    store = torch.rand((3, 6, 7))
    rec = store.transpose(1, 2)                                     # (3, 7, 6), strides (42, 1, 7)
    valid = rec[..., 5] > 0.5
    D.tag_record(rec, valid)
    _falls_back(*_views(rec), valid, rec)


def test_valid_edited_after_tagging_falls_back():
    rec, valid = _record(7)
    D.tag_record(rec, valid)
    valid[0, 0] = not bool(valid[0, 0])
    _falls_back(*_views(rec), valid, rec)


def test_base_edited_after_tagging_falls_back():
    rec, valid = _record(8)
    D.tag_record(rec, valid)
    rec[0, 0, 5] = 1.0 - rec[0, 0, 5]                               # now rec[..., 5] contradicts valid
    _falls_back(*_views(rec), valid, rec)
    rec, valid = _record(9)
    D.tag_record(rec, valid)
    mk1, mk2, scores = _views(rec)
    scores.mul_(2.0)                                                # through a view: the same version counter
    _falls_back(mk1, mk2, scores, valid, rec)


def test_plain_tensors_as_before():
    g = torch.Generator().manual_seed(10)
    mk1, mk2 = torch.rand((2, 5, 2), generator=g), torch.rand((2, 5, 2), generator=g)
    scores, valid = torch.rand((2, 5), generator=g), torch.rand((2, 5), generator=g) > 0.5
    got = D.pack_records(mk1, mk2, scores, valid)
    assert got.shape == (2, 5, 6) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, _slow(mk1, mk2, scores, valid))
