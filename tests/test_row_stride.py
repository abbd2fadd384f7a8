"""hip_autograd._uniform_row_stride against brute force.

The helper decides whether gatemul reads an operand in place through
one row stride or pays a contiguous() copy.  A wrong non-None answer
makes the kernel read the wrong rows, so: whenever it returns a stride,
that stride must be THE uniform row stride of t.reshape(-1, C)'s element
addresses; where no uniform stride exists it must return None.  None
where a stride exists is allowed (costs a copy, stays correct).
"""
import pytest
import torch

from alphafold2_amd.ops.hip_autograd import _uniform_row_stride


def _brute_force(t):
    """(exists, stride): uniform row stride of the (rows, C) enumeration
    of t's element addresses; stride is None when any value fits (one
    row)."""
    C = t.shape[-1]
    n = t.untyped_storage().nbytes() // t.element_size()
    addr = torch.as_strided(torch.arange(n), t.size(), t.stride(),
                            t.storage_offset()).reshape(-1, C)
    if C > 1 and not (addr[:, 1:] - addr[:, :-1] == 1).all():
        return False, None
    starts = addr[:, 0]
    if starts.numel() == 1:
        return True, None
    steps = starts[1:] - starts[:-1]
    if not (steps == steps[0]).all():
        return False, None
    return True, int(steps[0])


def _layouts():
    b = torch.zeros(4, 6, 5, 16)
    return {
        'contiguous': b,
        'narrow_last': b.narrow(-1, 4, 8),
        'narrow_last_odd': b.narrow(-1, 3, 5),
        'batch_slice': b[1:3],
        'row_slice': b[:, :, 1:4],
        'row_slice_narrow': b[:, :, 1:4, 8:],
        'row_step': b[:, :, ::2],
        'middle_step': b[:, ::2],
        'middle_slice': b[:, 1:4],
        'batch_step': b[::2],
        'permuted_outer': b.permute(1, 0, 2, 3),
        'permuted_rows': b.permute(0, 2, 1, 3),
        'size1_dims': b[:1, :1],
        'size1_middle': b[:, 2:3],
        'size1_rows': b[:, :, 3:4],
        'size1_rows_narrow': b[:, :, 3:4, :8],
        'unsqueezed': b[0].unsqueeze(1),
        'expand_rows': b[:, :, :1].expand(4, 6, 5, 16),
        'expand_batch': b[:1].expand(3, 6, 5, 16),
        'expand_all': b[:1, :1, :1].expand(4, 6, 5, 16),
        'expand_last': b[..., :1].expand(4, 6, 5, 16),
        'one_d': torch.zeros(16),
        'one_d_slice': torch.zeros(32)[8:24],
        'one_d_step': torch.zeros(32)[::2],
        'two_d': torch.zeros(7, 16),
        'two_d_narrow': torch.zeros(7, 64).narrow(-1, 16, 16),
        'two_d_row_step': torch.zeros(8, 16)[::3],
        'two_d_one_row': torch.zeros(7, 64)[2:3, 8:24],
        'transposed_last': b.transpose(-1, -2),
        'two_d_transposed': torch.zeros(7, 16).t(),
        'last_step': b[..., ::2],
        'single_channel': torch.zeros(5, 3, 8)[..., 2:3],
        'chunk_half': torch.zeros(3, 9, 32).chunk(2, dim=-1)[1],
        'packed_gate': torch.zeros(2, 6, 9, 64).narrow(-1, 48, 16),
        'flattened_view': b.reshape(24, 5, 16)[:, 1:],
    }


@pytest.mark.parametrize("name", sorted(_layouts()))
def test_uniform_row_stride_matches_brute_force(name):
    t = _layouts()[name]
    got = _uniform_row_stride(t)
    exists, stride = _brute_force(t)
    if not exists:
        assert got is None, f"{name}: returned {got}, no uniform stride"
    elif got is not None and stride is not None:
        assert got == stride, f"{name}: returned {got}, rows step {stride}"


def test_uniform_row_stride_keeps_the_zero_copy_cases():
    """The layouts the model relies on must stay zero-copy (a None here
    is correct but would silently add a copy per gate)."""
    lay = _layouts()
    assert _uniform_row_stride(lay['contiguous']) == 16
    assert _uniform_row_stride(lay['narrow_last']) == 16
    assert _uniform_row_stride(lay['packed_gate']) == 64
    assert _uniform_row_stride(lay['chunk_half']) == 32
    assert _uniform_row_stride(lay['two_d_narrow']) == 64
