"""tests/kernel_abi.py itself, on CPU tensors: the alignment the two operand layouts rest on, a guard check that fires for a
write on either side of an output AND of an input, and the comparison helpers."""
import math

import numpy as np
import pytest
import torch

from kernel_abi import F32, F64, GUARD, I64, SENTINEL, Arena, covered, ptr, same_bits, sfx, unit, untouched

NAN = float("nan")
DTYPES = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64"), pytest.param(I64, id="i64")]
# (fill, dtype) of the guard-violation cases: the sentinel, flow's NaN, an integer buffer
FILLS = [pytest.param(SENTINEL, F32, id="777"), pytest.param(NAN, F64, id="nan"), pytest.param(SENTINEL, I64, id="i64")]


@pytest.mark.parametrize("dtype", DTYPES)
def test_shift_0_is_16_byte_aligned_and_shift_1_is_not(dtype):
    """shift 0 is what sends a case down the kernels' 16-byte path, shift 1 down their element path"""
    item = torch.empty(0, dtype=dtype).element_size()
    for shift, rest in ((0, 0), (1, (GUARD + 1) * item % 16)):
        ar = Arena(shift, device="cpu")
        views = [ar.put(torch.arange(5).to(dtype)), ar.put(np.arange(6.0).reshape(2, 3), dtype), ar.out(7, dtype), ar.out((2, 3), dtype)]
        assert [v.data_ptr() % 16 for v in views] == [rest] * 4
        assert rest == (0 if shift == 0 else {4: 4, 8: 8}[item])
        assert [tuple(v.shape) for v in views] == [(5,), (2, 3), (7,), (2, 3)]


def test_put_and_out_take_their_dtype_from_the_call_then_the_arena_then_the_tensor():
    ar = Arena(dtype=F64, device="cpu")
    x = torch.tensor([1.5, -2.0], dtype=F32)
    assert ar.put(x).dtype == F64 and ar.put(x, F32).dtype == F32 and ar.out(3).dtype == F64 and ar.out(3, I64).dtype == I64
    assert ar.put(None) is None and torch.equal(ar.put(x), x.double())
    assert Arena(device="cpu").put(x).dtype == F32
    assert untouched(ar.out(3)) and untouched(ar.out(3, I64)) and ar.out(3, I64)[0].item() == 777
    with pytest.raises(ValueError):
        Arena(fill=NAN, device="cpu").out(3, I64)


@pytest.mark.parametrize("fill,dtype", FILLS)
@pytest.mark.parametrize("shift", [0, 1])
def test_check_guards_fires_for_one_element_on_either_side_of_an_output_and_of_an_input(fill, dtype, shift):
    def arena():
        ar = Arena(shift, fill=fill, dtype=dtype, device="cpu")
        ar.put(torch.arange(5))
        ar.out((2, 3)).fill_(1)          # (a kernel writing all of its output)
        return ar
    arena().check_guards()
    for which in (0, 1):                                  # the input, the output
        for side in ("before", "after"):
            ar = arena()
            buf, o, n = ar.bufs[which]                    # the arena's own backing tensor: the write stays inside it
            buf[o - 1 if side == "before" else o + n] = 5
            with pytest.raises(AssertionError, match="write outside the tensor"):
                ar.check_guards()
            ar = arena()
            buf, o, n = ar.bufs[which]
            buf[0 if side == "before" else -1] = 5        # the far ends of the guards
            with pytest.raises(AssertionError):
                ar.check_guards()


@pytest.mark.parametrize("fill,dtype", FILLS)
def test_untouched_and_covered_flip_after_one_element(fill, dtype):
    ar = Arena(fill=fill, dtype=dtype, device="cpu")
    a, b = ar.out(4), ar.out((2, 2))
    assert ar.untouched() and untouched(a, fill) and untouched(b, fill)
    with pytest.raises(AssertionError):
        covered([a], fill)
    a.fill_(3)
    covered([a, None], fill)
    a[2] = fill if dtype != I64 else int(fill)
    with pytest.raises(AssertionError):
        covered([a], fill)
    assert not ar.untouched() and not untouched(a, fill) and untouched(b, fill)
    ar = Arena(fill=fill, dtype=dtype, device="cpu")
    ar.out(4)
    ar.bufs[0][0][0] = 3                                  # a guard element counts: a rejected call writes nothing at all
    assert not ar.untouched()


def test_same_bits():
    for dtype in (F32, F64):
        assert not same_bits(torch.tensor([0.0], dtype=dtype), torch.tensor([-0.0], dtype=dtype))
        nan = torch.tensor([NAN, 1.0], dtype=dtype)
        assert same_bits(nan, nan.clone())
        assert not same_bits(nan, -nan)                   # another NaN payload (the sign bit)
        x = torch.arange(6, dtype=dtype)
        assert same_bits(x, x.clone()) and same_bits(x.view(2, 3).t(), x.view(2, 3).t().contiguous())
        assert not same_bits(x, x.view(2, 3)) and not same_bits(x, x + 1)
    assert not same_bits(torch.zeros(2, dtype=F32), torch.zeros(2, dtype=F64))
    i = torch.tensor([1, 1 << 40, -3])
    assert same_bits(i, i.clone()) and not same_bits(i, i + 1) and not same_bits(i, i.view(3, 1))
    assert same_bits(None, None) and not same_bits(None, i) and not same_bits(i, None)


def test_ptr_sfx_unit():
    t = torch.zeros(3)
    assert ptr(None) is None and ptr(1234) == 1234 and ptr(t) == t.data_ptr() and ptr(t[1:]) == t.data_ptr() + 4
    assert sfx(F32) == "_f32" and sfx(F64) == "_f64"
    assert unit(F32) == math.ldexp(1.0, -24) and unit(F64) == math.ldexp(1.0, -53)
