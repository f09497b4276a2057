"""tests/guarded.py can fail: every way a kernel may leave its operand -- one float in front, one behind, a pad column, a guard
float replaced by another NaN, an input changed in its last bit -- is rejected by intact() or keeps(); a clean operand passes."""
import pytest
import torch

from tests.guarded import GUARD_BITS, Guarded, GuardedSet, band_floats, canary

ROWS, COLS, LD = 5, 12, 16


def make(ld=LD):
    g = torch.Generator().manual_seed(3)
    return Guarded(ROWS, COLS, ld, fill=torch.randn(ROWS, COLS, generator=g), device="cpu")


def test_a_clean_operand_passes():
    for ld in (COLS, LD):
        t = make(ld)
        assert t.ptr % 16 == 0 and t.band == band_floats(ld) >= max(1024, 128 * ld)
        assert t.intact() and t.keeps() and t.first_damage() is None
        assert t.region.shape == (ROWS, COLS) and not t.region.isnan().any()
        assert int((t.buf.view(torch.int32) == GUARD_BITS).sum()) == 2 * t.band + (ROWS - 1) * (ld - COLS)
        t.region.mul_(2.0)                      # writing the operand itself is no damage
        assert t.intact() and not t.keeps()
        t.check("clean", written=True)


def test_outputs_start_as_nan_and_the_canary_alternates():
    out = Guarded(ROWS, COLS, LD, device="cpu")
    assert out.region.isnan().all() and not bool((out.region.contiguous().view(torch.int32) == GUARD_BITS).any())
    with pytest.raises(AssertionError, match=r"NaN left at \(0, 0\)"):
        out.check("unwritten", written=True)
    c = canary(3, 4).view(-1)
    assert c[0::2].isnan().all() and bool((c[1::2] == torch.tensor(12345.678)).all())
    keep = Guarded(3, 4, 8, fill=canary(3, 4), device="cpu")
    assert keep.keeps()
    keep.region[2, 3] += 1.0                    # an accumulation onto the finite half shows
    assert not keep.keeps()


@pytest.mark.parametrize("ld", [COLS, LD])
def test_one_float_in_front_of_the_region_is_seen(ld):
    t = make(ld)
    t.buf[t.band - 1] = 0.0
    assert not t.intact()
    assert t.first_damage() == ("front", -1, ld - 1)
    with pytest.raises(AssertionError, match="front band, row -1"):
        t.check("front")


@pytest.mark.parametrize("ld", [COLS, LD])
def test_one_float_behind_the_region_is_seen(ld):
    t = make(ld)
    t.buf[t.band + t.span] = 1.0
    assert not t.intact()
    band, row, col = t.first_damage()
    assert band == "behind" and (row, col) == ((ROWS, 0) if ld == COLS else (ROWS - 1, COLS))


def test_one_pad_column_is_seen():
    t = make()
    t.buf[t.band + 2 * LD + COLS + 1] = 3.0
    assert not t.intact()
    assert t.first_damage() == ("pad", 2, COLS + 1)


def test_a_guard_float_replaced_by_another_nan_is_seen():
    for where in (lambda t: 7, lambda t: t.band + LD + COLS, lambda t: t.buf.numel() - 1):
        t = make()
        t.buf[where(t)] = float("nan")          # the regular NaN: not the guard's payload
        assert t.buf.isnan()[where(t)] and not t.intact()


def test_the_gap_between_two_slabs_is_guarded():
    t = Guarded(3, 4, 6, fill=torch.arange(24.0).view(2, 3, 4), device="cpu", slabs=2, slab_stride=40)
    assert t.region.shape == (2, 3, 4) and t.intact() and t.keeps()
    assert float(t.buf[t.band + 40 + 6 + 1]) == 17.0          # slab 1, row 1, column 1
    t.buf[t.band + 16] = 0.0                                   # the first float behind slab 0's last row
    assert t.first_damage() == ("pad", 2, 4)
    t = Guarded(3, 4, 6, device="cpu", slabs=2, slab_stride=40)
    t.buf[t.band + 40 + 16] = 0.0                              # ... and behind slab 1's
    assert t.first_damage() == ("behind", 2, 4)


def test_an_input_changed_in_its_last_bit_is_seen():
    t = make()
    t.region.view(torch.int32)[ROWS - 1, COLS - 1] ^= 1
    assert t.intact() and not t.keeps()
    with pytest.raises(AssertionError, match="changed"):
        t.check("input", unchanged=True)


def test_a_set_checks_inputs_for_their_bits_and_outputs_for_their_bands():
    s = GuardedSet(device="cpu")
    a, o = s.inp("a", torch.arange(6.0).view(2, 3), ld=4), s.out("o", 2, 3, ld=7)
    o.region.fill_(1.0)
    s.check()
    a.region[0, 0] = 9.0
    with pytest.raises(AssertionError, match="input a: changed"):
        s.check()
    a.region[0, 0] = 0.0
    o.buf[o.band + 3] = 0.0
    with pytest.raises(AssertionError, match="output o: wrote outside"):
        s.check()
