"""The placement helper itself (tests/_placed.py) on CPU tensors: the residues it promises and what its guard check sees."""
import pytest
import torch
from _placed import GUARD, LINE, SENTINEL, assert_guards, assert_residue, assert_unchanged, place, placed_like

DTYPES = [torch.uint8, torch.int8, torch.int32, torch.int64, torch.float32, torch.float64]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_place_yields_every_legal_residue(dtype):
    item = torch.empty((), dtype=dtype).element_size()
    for offset in range(0, LINE, item):
        view, h = place((3, 5), dtype, offset, device="cpu")
        assert view.data_ptr() % LINE == offset and h.buf.data_ptr() % LINE == 0
        assert view.shape == (3, 5) and view.dtype is dtype and view.is_contiguous()
        assert h.buf.numel() == GUARD + LINE + 15 * item + GUARD and h.start == GUARD + offset and h.nbytes == 15 * item
        assert bool((h.buf == SENTINEL).all())
        assert_residue(view, offset, item, "view")
        assert_guards(h, "view")
    for bad in (-item, LINE, 1 if item > 1 else LINE + 1):
        with pytest.raises(AssertionError):
            place((3, 5), dtype, bad, device="cpu")


def test_a_view_writes_its_own_bytes_only():
    view, h = place((7, 3), torch.float32, 20, device="cpu")
    view.zero_()
    assert_guards(h, "view")
    assert int((h.buf != SENTINEL).sum()) == 7 * 3 * 4 and bool((h.body() == 0).all())


def test_a_byte_in_front_or_behind_is_reported_and_one_inside_is_not():
    for offset in (0, 16, 112):
        view, h = place((4, 6), torch.float32, offset, device="cpu")
        h.buf[h.start] = 0                                   # first byte of the view
        h.buf[h.start + h.nbytes - 1] = 0                    # last byte of the view
        assert_guards(h, "obs")
        h.buf[h.start - 1] = 0
        with pytest.raises(AssertionError, match=r"IN FRONT of obs: offsets -1 \.\. -1 "):
            assert_guards(h, "obs")
        h.buf[h.start - 1] = SENTINEL
        h.buf[h.start + h.nbytes] = 0
        with pytest.raises(AssertionError, match=rf"BEHIND obs: offsets {h.nbytes} \.\. {h.nbytes} "):
            assert_guards(h, "obs")
        h.buf[h.start + h.nbytes] = SENTINEL
        h.buf[0] = 1
        h.buf[h.start - 112] = 1
        h.buf[-1] = 1
        with pytest.raises(AssertionError) as e:
            assert_guards(h, "obs")
        msg = str(e.value)
        assert f"placed at +{offset}" in msg and f"offsets {-h.start} .. -112 " in msg
        last = h.buf.numel() - 1 - h.start
        assert f"offsets {last} .. {last} " in msg


def test_placed_like_copies_and_notices_a_changed_input():
    src = torch.arange(35, dtype=torch.float64).reshape(5, 7)
    view, h = placed_like(src, 8)
    assert view.data_ptr() % LINE == 8 and torch.equal(view, src)
    assert_unchanged(h, src, "reward")
    view[2, 3] = -1.0
    with pytest.raises(AssertionError, match="input reward placed at \\+8 was written"):
        assert_unchanged(h, src, "reward")
    src8 = torch.arange(11, dtype=torch.uint8)
    v8, h8 = placed_like(src8, 1)
    assert v8.data_ptr() % LINE == 1 and torch.equal(v8, src8)
    assert_unchanged(h8, src8, "actions")


def test_residue_assertion_rejects_another_address():
    view, _ = place((4,), torch.float32, 16, device="cpu")
    with pytest.raises(AssertionError, match="wanted \\+32"):
        assert_residue(view, 32, 16, "obs")
    v4, _ = place((4,), torch.float32, 4, device="cpu")
    with pytest.raises(AssertionError, match="16-byte alignment"):
        assert_residue(v4, 4, 16, "obs")
