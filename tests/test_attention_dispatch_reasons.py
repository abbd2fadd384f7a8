"""The eager-fallback reason of the attention dispatch names the
predicate that actually failed (no GPU needed: the extension is faked)."""
import types
from unittest import mock

import torch

from alphafold2_amd.ops import dispatch

FULL = types.SimpleNamespace(attn_fwd=None, attn_bwd=None,
                             attn_dropout_mask=None)
NO_DROP = types.SimpleNamespace(attn_fwd=None, attn_bwd=None)
NO_ATTN = types.SimpleNamespace(layernorm_fwd=None)


def _reason(ext, dtype=torch.bfloat16, dim_head=64, bias=None, drop_p=0.,
            tie_dim=None, batch=6):
    q = torch.zeros(batch, 2, 8, dim_head, dtype=dtype)
    with mock.patch.object(dispatch, '_load_ext', return_value=ext):
        return dispatch._attn_unfusable_reason(q, dim_head, bias, drop_p,
                                               tie_dim, batch)


def test_covered_configurations_have_no_reason():
    assert _reason(FULL) is None
    assert _reason(FULL, drop_p=0.25) is None
    assert _reason(FULL, dim_head=32, tie_dim=3) is None
    assert _reason(NO_DROP) is None          # dropout off: mask dump unused
    assert _reason(None, drop_p=0.25) is None  # no extension: not judged here


def test_each_failed_predicate_is_named():
    assert _reason(NO_ATTN) == 'extension built without attn_fwd'
    r = _reason(NO_DROP, drop_p=0.25)
    assert 'dropout active' in r and 'without attn_dropout_mask' in r
    assert 'p=1.0' in _reason(FULL, drop_p=1.0)
    assert _reason(FULL, dim_head=72) == \
        'dim_head=72 (fused kernel covers multiples of 8 up to 64)'
    assert _reason(FULL, dim_head=20).startswith('dim_head=20 ')
    assert _reason(FULL, dtype=torch.float32) == \
        'dtype=torch.float32 (fused kernel is bf16)'
    assert _reason(FULL, bias=torch.zeros(1)) == \
        'bias dtype=torch.float32 (fused kernel is bf16)'
    assert _reason(FULL, tie_dim=4, batch=6) == \
        'batch 6 is not divisible by tie_dim=4'
    # dropout on a configuration that fails for another reason names
    # that reason, not the dropout
    assert _reason(FULL, dim_head=72, drop_p=0.25).startswith('dim_head=72')
