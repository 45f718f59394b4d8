"""The poison mode's host side (ops.set_poison / ops.empty / ops.check_guards, _lib.set_dirty_lds) on CPU tensors: what the GPU
poison pass (tests/test_gpu_poison.py) relies on.  The guard bands are checked by writing through the registry's base tensor:
base[G - 1] is the last byte below the view, base[G + n] the first byte above it."""
import pytest
import torch

from grl_image_restoration_amd import _lib, ops

G = ops.GUARD_BYTES


@pytest.fixture
def guards():
    prev = ops.set_poison(True, guards=True)
    try:
        yield
    finally:
        ops.set_poison(prev)
        ops._GUARDED.clear()


def test_guard_band_is_the_red_zone_of_poison_alloc_and_keeps_alignment(guards):
    assert G == 4096
    for shape, dt in (((3, 5), torch.float32), ((7,), torch.uint8), ((2, 3, 5), torch.float16), ((1,), torch.float64)):
        t = ops.empty(*shape, dtype=dt, device="cpu")
        base = ops._GUARDED[-1][0]
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()
        assert t.data_ptr() == base.data_ptr() + G and t.data_ptr() % 16 == 0
        assert base.numel() >= t.numel() * t.element_size() + 2 * G
    assert ops.empty((4, 2), dtype=torch.float32, device="cpu").shape == (4, 2)      # a shape tuple, as torch.empty takes it
    ops.check_guards()


@pytest.mark.parametrize("shape,dtype", [((3, 5), torch.float32), ((13,), torch.uint8), ((5, 3), torch.float16)])
@pytest.mark.parametrize("side", ["below", "above"])
def test_a_write_next_to_the_view_is_reported_with_side_and_shape(guards, shape, dtype, side):
    quiet = ops.empty(9, dtype=torch.float32, device="cpu")
    t = ops.empty(*shape, dtype=dtype, device="cpu")
    base, n = ops._GUARDED[-1][0], t.numel() * t.element_size()
    base[G - 1 if side == "below" else G + n] = 0
    with pytest.raises(AssertionError) as e:
        ops.check_guards()
    msg = str(e.value)
    assert str(tuple(shape)) in msg and str(dtype) in msg and f"{side} the tensor" in msg
    assert ("above" if side == "below" else "below") not in msg
    assert "(9,)" not in msg and quiet is not None                   # the untouched neighbour is not named
    assert ops._GUARDED == []                                        # cleared, also after a finding
    ops.check_guards()


def test_writes_inside_the_view_are_not_reported_and_the_registry_is_cleared(guards):
    t = ops.empty(3, 5, dtype=torch.float32, device="cpu")
    u = ops.empty_like(torch.zeros(6, 2, dtype=torch.float16))
    b = ops.empty(11, dtype=torch.uint8, device="cpu")
    assert len(ops._GUARDED) == 3
    t.fill_(1.0), u.fill_(2.0), b.fill_(0)
    t[0, 0], t[-1, -1], b[0], b[-1] = -3.0, 7.0, 255, 255
    base, n = ops._GUARDED[0][0], t.numel() * 4
    base[G], base[G + n - 1] = 0, 0                                  # the first and the last byte of the view
    ops.check_guards()
    assert ops._GUARDED == []
    nc = torch.zeros(4, 6).t()                                       # non-contiguous: falls back to no guards, still poisoned
    v = ops.empty_like(nc)
    assert ops._GUARDED == [] and v.stride() == nc.stride() and bool(torch.isnan(v).all())


def test_poison_off_is_a_plain_torch_empty():
    assert not ops._POISON and not ops._GUARDS
    t = ops.empty(3, 5, dtype=torch.float32, device="cpu")
    assert t.storage_offset() == 0 and t.untyped_storage().nbytes() == 3 * 5 * 4
    e = ops.empty_like(torch.zeros(4, 6).t())
    assert e.storage_offset() == 0 and e.stride() == (1, 6)
    assert ops._GUARDED == []
    ops.check_guards()                                               # nothing registered: nothing to do
    prev = ops.set_poison(True)                                      # poison without guards: today's GRL_POISON=1
    try:
        t = ops.empty(3, 5, dtype=torch.float32, device="cpu")
        assert t.storage_offset() == 0 and ops._GUARDED == [] and bool(torch.isnan(t).all())
    finally:
        ops.set_poison(prev)


@pytest.mark.parametrize("with_guards", [False, True])
def test_poison_values(with_guards):
    prev = ops.set_poison(True, guards=with_guards)
    try:
        for dt in (torch.float64, torch.float32, torch.float16):
            assert bool(torch.isnan(ops.empty(5, 3, dtype=dt, device="cpu")).all())
        assert bool((ops.empty(37, dtype=torch.uint8, device="cpu") == 0x7F).all())
        assert bool((ops.empty(4, dtype=torch.int32, device="cpu") == 0x7F7F7F7F).all())
        assert ops.empty(0, 4, dtype=torch.float32, device="cpu").shape == (0, 4)
        if with_guards:
            for base, n, _, _ in ops._GUARDED:                      # the bands hold the pattern, right up to the view
                assert bool((base[:G] == ops.GUARD_BYTE).all()) and bool((base[G + n:] == ops.GUARD_BYTE).all())
                assert base.numel() - G - n >= G
        ops.check_guards()
    finally:
        ops.set_poison(prev)
        ops._GUARDED.clear()


def test_switches_return_the_previous_value_and_restore_it():
    assert ops.set_poison(True) is False
    assert ops.set_poison(True, guards=True) is True and ops._GUARDS
    assert ops.set_poison(False) is True
    assert not ops._POISON and not ops._GUARDS                       # switching poison off switches the guards off
    assert ops.set_poison(False, guards=True) is False and not ops._GUARDS    # no guards without poison
    assert _lib.set_dirty_lds(True) is False
    assert _lib._DIRTY_LDS is True
    assert _lib.set_dirty_lds(False) is True
    assert _lib._DIRTY_LDS is False and _lib.set_dirty_lds(False) is False
