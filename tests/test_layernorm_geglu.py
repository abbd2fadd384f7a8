"""layernorm.hip and geglu.hip against the float64 formulas, over every
instantiation the host launchers can select (dtype, vector width, GROUP,
MAXCHUNK, row packing, grid-stride loops, the past-16-chunks tail).

Elementwise bound |got - ref64| <= T * |ref64| + c * S + 1e-6 with
T = 2**-8 (bf16) / 2**-10 (fp16) / 1e-5 (fp32), twice the output
rounding, and S the float64 sum of the absolute values of the terms that
cancel (c = 1e-5 for fp32 sums, 1e-6 for the erf / exp of gelu).  The
reference always starts from the rounded inputs the kernel reads.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10,
       torch.float32: 1e-5}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
EPS = 1e-5


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


def _assert_bound(name, got, ref, bound):
    assert got.shape == ref.shape, name
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)                      # NaN counts as off
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements off, worst "
        f"err/bound {(err / bound).max().item():.3g}, max err "
        f"{err.max().item():.3e}")


# ---------------------------------------------------------------------------
# layernorm


def _ln_ref(x, w, b, dy):
    """float64 forward, backward and the bound terms of each output."""
    x, w, b, dy = x.double(), w.double(), b.double(), dy.double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    rs = (var + EPS).rsqrt()
    xh = (x - mean) * rs
    g = dy * w
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * xh).mean(-1, keepdim=True)
    return dict(
        y=xh * w + b, S_y=(xh * w).abs() + b.abs(),
        dx=rs * (g - c1 - xh * c2),
        S_dx=rs * (g.abs() + c1.abs() + (xh * c2).abs()),
        dw=(dy * xh).sum(0), S_dw=(dy * xh).abs().sum(0),
        db=dy.sum(0), S_db=dy.abs().sum(0),
        mean=mean.squeeze(-1), S_mean=x.abs().mean(-1), rstd=rs.squeeze(-1))


def _ln_check(ext, x, w, b, dy, w_round=0.0):
    dtype = x.dtype
    y, mean, rstd = ext.layernorm_fwd(x, w, b, EPS)
    dx, dw, db = ext.layernorm_bwd(dy, x, w, mean, rstd)
    assert y.dtype == dtype and dx.dtype == dtype
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32
    assert dw.dtype == w.dtype and db.dtype == w.dtype
    r = _ln_ref(x, w, b, dy)
    T = TOL[dtype]
    _assert_bound("mean", mean, r['mean'], 1e-5 * r['S_mean'] + 1e-6)
    _assert_bound("rstd", rstd, r['rstd'], 1e-5 * r['rstd'])
    _assert_bound("y", y, r['y'], T * r['y'].abs() + 1e-5 * r['S_y'] + 1e-6)
    _assert_bound("dx", dx, r['dx'],
                  T * r['dx'].abs() + 1e-5 * r['S_dx'] + 1e-6)
    _assert_bound("dw", dw, r['dw'],
                  w_round * r['dw'].abs() + 1e-5 * r['S_dw'] + 1e-6)
    _assert_bound("db", db, r['db'],
                  w_round * r['db'].abs() + 1e-5 * r['S_db'] + 1e-6)


def _ln_inputs(rows, D, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, D, device=DEV, generator=g).to(dtype)
    dy = torch.randn(rows, D, device=DEV, generator=g).to(dtype)
    w = torch.randn(D, device=DEV, generator=g) * 0.5 + 1
    b = torch.randn(D, device=DEV, generator=g) * 0.1
    return x, w, b, dy


# Reached instantiation <VEC, GROUP, MAXCHUNK>, for 2-byte types | fp32
# (VEC 8 | 4 when D divides, else 1; "lds" = LDS combine of dw/db,
# "atom" = atomics into the block's partial row, "tail" = columns past the
# 16 register-held chunks):
LN_SHAPES = [
    (1, 8),       # <8,16,1> lds | <4,16,1> lds, one row, one block
    (37, 64),     # <8,16,1> lds | <4,16,1> lds
    (37, 128),    # <8,16,1> lds | <4,32,1> lds
    (130, 256),   # <8,32,1> lds | <4,64,1> lds, several blocks
    (7, 33),      # <1,64,1> lds | <1,64,1> lds
    (130, 264),   # <8,64,1> lds | <4,64,4> atom
    (66, 1032),   # <8,64,4> atom | <4,64,16> atom
    (5, 1536),    # <8,64,4> atom | <4,64,16> atom
    (3, 1026),    # <1,64,16> atom + tail of 2 columns, a single block
    (9, 1026),    # the same with three blocks
    (3, 4100),    # <1,64,16> tail of 3076 | <4,64,16> tail of one vec4
]


@pytest.mark.parametrize("rows,D", LN_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_fwd_bwd(ext, dtype, rows, D):
    _ln_check(ext, *_ln_inputs(rows, D, dtype))


# (8200, 264): 4 rows per block, 2048 blocks -> first round ends at row
# 8192; (33000, 8): 16 rows per block -> 32768.
@pytest.mark.parametrize("rows,D,first_round", [(8200, 264, 8192),
                                                (33000, 8, 32768)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_grid_stride(ext, dtype, rows, D, first_round):
    """More rows than one round of the capped grid.  dy is nonzero in six
    rows only (first, last, two on each side of the round boundary), so a
    dropped or doubled row moves dw/db by a whole term."""
    x, w, b, dy = _ln_inputs(rows, D, dtype, seed=1)
    keep = torch.tensor([0, first_round - 2, first_round - 1, first_round,
                         first_round + 1, rows - 1], device=DEV)
    sparse = torch.zeros_like(dy)
    sparse[keep] = dy[keep]
    _ln_check(ext, x, w, b, sparse)


def test_layernorm_dispatch_strided_bf16_weights(ext):
    """dispatch.layer_norm as the model calls it: x and dy are views with
    padded rows, weight and bias are bf16 (so dw/db carry one more output
    rounding)."""
    from alphafold2_amd.ops import dispatch
    rows, D = 37, 128
    g = torch.Generator(device=DEV).manual_seed(2)
    mk = lambda *s: torch.randn(*s, device=DEV, generator=g) \
        .to(torch.bfloat16)
    xbase, dybase = mk(rows, D + 8), mk(rows, 2 * D)
    w0, b0 = (mk(D) * 0.5 + 1), mk(D) * 0.1
    x = xbase[:, 3:3 + D].detach().requires_grad_(True)
    dy = dybase[:, ::2]
    assert not x.is_contiguous() and not dy.is_contiguous()
    w = w0.clone().requires_grad_(True)
    b = b0.clone().requires_grad_(True)
    y = dispatch.layer_norm(x, w, b, EPS)
    y.backward(dy)

    r = _ln_ref(x.detach(), w0, b0, dy)
    T = TOL[torch.bfloat16]
    _assert_bound("y", y.detach(), r['y'],
                  T * r['y'].abs() + 1e-5 * r['S_y'] + 1e-6)
    _assert_bound("dx", x.grad, r['dx'],
                  T * r['dx'].abs() + 1e-5 * r['S_dx'] + 1e-6)
    assert w.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16
    _assert_bound("dw", w.grad, r['dw'],
                  T * r['dw'].abs() + 1e-5 * r['S_dw'] + 1e-6)
    _assert_bound("db", b.grad, r['db'],
                  T * r['db'].abs() + 1e-5 * r['S_db'] + 1e-6)


@pytest.mark.parametrize("offset,spread", [(30.0, 0.1), (100.0, 0.05)])
@pytest.mark.parametrize("D", [33, 256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm_offset_rows(ext, dtype, D, offset, spread):
    """Rows whose mean dwarfs their spread, where sumsq / D - mean**2 in
    fp32 loses the variance (13 % off at 30 + 0.1 randn, negative in 19
    of 64 rows at 100 + 0.05 randn, D = 256).

    What fp32 can deliver here is limited by the rounding of the mean, so
    the bound is measured, not fixed: the max error of PyTorch's own fp32
    layer_norm against float64 on the same inputs, times 4 for a different
    but still stable summation order, plus the output rounding T * |ref|
    for bf16.  Measured max |y - ref64| in fp32 for the offsets 30 / 100:
    PyTorch on a CPU 2.6e-5 / 2.6e-4, PyTorch on the MI355X 5.9e-5 /
    4.2e-4, this kernel 1.2e-6 / 1.6e-6 (it normalises x - x[0] minus the
    shifted mean, so the rounding of the mean never enters y); dx, which
    uses the stored fp32 mean like PyTorch does: PyTorch 3.2e-4 / 3.5e-3,
    kernel 1.1e-4 / 1.4e-3.
    Row 0 is the constant 1000: its output is exactly the bias."""
    rows = 64
    g = torch.Generator(device=DEV).manual_seed(3)
    x = (offset + spread * torch.randn(rows, D, device=DEV, generator=g))
    x[0] = 1000.0
    x = x.to(dtype)
    dy = torch.randn(rows, D, device=DEV, generator=g).to(dtype)
    w = torch.randn(D, device=DEV, generator=g) * 0.5 + 1
    b = torch.randn(D, device=DEV, generator=g) * 0.1

    r = _ln_ref(x, w, b, dy)
    xt = x.float().requires_grad_(True)
    yt = F.layer_norm(xt, (D,), w, b, EPS)
    yt.backward(dy.float())
    torch_y = (yt.detach().double() - r['y']).abs().max().item()
    # dx without the constant row, where rstd = eps**-0.5 multiplies any
    # last-bit difference in its variance by 316
    torch_dx = (xt.grad.double() - r['dx'])[1:].abs().max().item()
    assert torch_y < 1e-2 and torch_dx < 1e-1          # a usable yardstick

    y, mean, rstd = ext.layernorm_fwd(x, w, b, EPS)
    dx, dw, db = ext.layernorm_bwd(dy, x, w, mean, rstd)
    for name, t in (('y', y), ('mean', mean), ('rstd', rstd), ('dx', dx),
                    ('dw', dw), ('db', db)):
        assert torch.isfinite(t).all(), f"{name} has NaN or Inf"
    assert (rstd > 0).all() and (rstd <= EPS ** -0.5 * (1 + 1e-6)).all()
    assert torch.equal(y[0].float(), b.to(dtype).float()), "constant row"
    T = TOL[dtype] if dtype != torch.float32 else 0.0
    got_y = (y.double() - r['y']).abs().max().item()
    got_dx = (dx.double() - r['dx'])[1:].abs().max().item()
    print(f"\noffset rows {dtype} D={D} offset={offset}: y err kernel "
          f"{got_y:.3e} torch fp32 {torch_y:.3e}; dx err kernel "
          f"{got_dx:.3e} torch fp32 {torch_dx:.3e}")
    _assert_bound("y", y, r['y'], T * r['y'].abs() + 4 * torch_y)
    _assert_bound("dx", dx[1:], r['dx'][1:],
                  T * r['dx'][1:].abs() + 4 * torch_dx)


# ---------------------------------------------------------------------------
# geglu


def _gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.5 ** 0.5))


def _gelu_grad64(g):
    cdf = 0.5 * (1.0 + torch.erf(g * 0.5 ** 0.5))
    pdf = torch.exp(-0.5 * g * g) * 0.3989422804014327
    return cdf + g * pdf


def _geglu_ref(x, dy):
    a, g = x.double().chunk(2, dim=-1)
    dy = dy.double()
    w = 1 + g.abs()
    return dict(y=a * _gelu64(g), S_y=a.abs() * w,
                da=dy * _gelu64(g), S_da=dy.abs() * w,
                dg=dy * a * _gelu_grad64(g), S_dg=(dy * a).abs() * w)


def _geglu_bounds(r, T):
    return {k: T * r[k].abs() + 1e-6 * r['S_' + k] + 1e-6
            for k in ('y', 'da', 'dg')}


def _geglu_check(ext, x, dy):
    H = dy.shape[-1]
    y = ext.geglu_fwd(x)
    dx = ext.geglu_bwd(dy, x)
    assert y.dtype == x.dtype and y.shape == dy.shape
    assert dx.dtype == x.dtype and dx.shape == x.shape
    r = _geglu_ref(x, dy)
    bd = _geglu_bounds(r, TOL[x.dtype])
    _assert_bound("y", y, r['y'], bd['y'])
    _assert_bound("da", dx[..., :H], r['da'], bd['da'])
    _assert_bound("dg", dx[..., H:], r['dg'], bd['dg'])


def _geglu_inputs(rows, H, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, 2 * H, device=DEV, generator=g).to(dtype)
    dy = torch.randn(rows, H, device=DEV, generator=g).to(dtype)
    return x, dy


def _gate_sweep(dtype):
    """One row, gate = linspace(-8, 8): both gelu tails and the middle."""
    H = 264
    g = torch.Generator(device=DEV).manual_seed(5)
    a = torch.randn(1, H, device=DEV, generator=g)
    gate = torch.linspace(-8, 8, H, device=DEV).reshape(1, H)
    dy = torch.randn(1, H, device=DEV, generator=g).to(dtype)
    return torch.cat([a, gate], dim=-1).to(dtype), dy


def test_geglu_bounds_hold_for_eager_fp32():
    """The bounds are only usable if plain fp32 arithmetic on this device
    stays inside them: check the eager fp32 formula and its autograd
    against float64 before relying on them for the kernel."""
    for x, dy in (_gate_sweep(torch.float32),
                  _geglu_inputs(37, 384, torch.float32)):
        H = dy.shape[-1]
        xt = x.clone().requires_grad_(True)
        a, g = xt.chunk(2, dim=-1)
        yt = a * F.gelu(g)
        yt.backward(dy)
        r = _geglu_ref(x, dy)
        bd = _geglu_bounds(r, TOL[torch.float32])
        _assert_bound("eager y", yt.detach(), r['y'], bd['y'])
        _assert_bound("eager da", xt.grad[..., :H], r['da'], bd['da'])
        _assert_bound("eager dg", xt.grad[..., H:], r['dg'], bd['dg'])


# Reached instantiation, for 2-byte types | fp32 (VEC; "packed r" = r rows
# per block iteration, "unpacked" = one row per block; columns per block
# step are 256 * VEC):
GEGLU_SHAPES = [
    (1, 8),       # VEC 8 unpacked (one chunk) | VEC 4 packed 128, 1 row
    (5, 64),      # VEC 8 packed 32 | VEC 4 packed 16, last iteration short
    (37, 256),    # VEC 8 packed 8 | VEC 4 packed 4, 37 % 8 and % 4 != 0
    (37, 384),    # VEC 8, 48 chunks, unpacked | VEC 4, 96 chunks, unpacked
    (3, 2048),    # VEC 8 unpacked, exactly one column step | VEC 4, two
    (3, 4096),    # VEC 8 two column steps | VEC 4 four
    (37, 12),     # VEC 4 (2-byte types: 8-byte lanes), 3 chunks, unpacked
    (37, 33),     # VEC 1 unpacked
    (66000, 8),   # VEC 8 unpacked: 66000 blocks wanted, capped at 65536,
                  # the rest by grid-stride | VEC 4 packed 128
]


@pytest.mark.parametrize("rows,H", GEGLU_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_fwd_bwd(ext, dtype, rows, H):
    _geglu_check(ext, *_geglu_inputs(rows, H, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_gate_sweep(ext, dtype):
    _geglu_check(ext, *_gate_sweep(dtype))


# H = 8: one chunk, unpacked; 384: 48 chunks, unpacked; 2048: the widest
# row the column-sum variant covers.  4099 rows: more than one row per
# block through the grid-stride loop of the resident grid.
@pytest.mark.parametrize("rows", [1, 4099])
@pytest.mark.parametrize("H", [8, 384, 2048])
def test_geglu_bwd_colsum(ext, H, rows):
    x, dy = _geglu_inputs(rows, H, torch.bfloat16, seed=6)
    dx, colsum = ext.geglu_bwd_colsum(dy, x)
    assert torch.equal(dx, ext.geglu_bwd(dy, x))
    assert colsum.dtype == torch.float32 and colsum.shape == (2 * H,)
    _assert_bound("colsum", colsum, dx.double().sum(0),
                  1e-5 * dx.double().abs().sum(0) + 1e-6)
