"""gatemul.hip (y = x * sigmoid(g) * rowmask) against the float64
formula and its analytic gradients, over every instantiation the host
launcher can select: dtype, vector width, GROUP, in-row loop, strided
operands, packed gradient writes and the grid-stride loop.

Elementwise bound |err| <= tol * |ref64| + 1e-6 with tol twice the
output-rounding half-ulp (2**-8 bf16, 2**-10 fp16) and, for fp32, the
project's fp32 kernel tolerance 1e-5 (covers __expf).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10,
       torch.float32: 1e-5}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


def _ref(x, g, dy, rm):
    """float64 (y, dx, dg); rm is a 0/1 per-row tensor or None."""
    x, g, dy = x.double(), g.double(), dy.double()
    m = torch.ones_like(x[..., :1]) if rm is None \
        else rm.double().reshape(*x.shape[:-1], 1)
    s = torch.sigmoid(g)
    return x * s * m, dy * m * s, dy * m * x * s * (1 - s)


def _assert_close(name, got, ref, dtype):
    assert got.dtype == dtype and got.shape == ref.shape, name
    err = (got.double() - ref).abs()
    bad = err > TOL[dtype] * ref.abs() + 1e-6
    assert not bad.any(), \
        f"{name}: {int(bad.sum())} elements off, max err {err.max().item():.3e}"


def _inputs(rows, C, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mk = lambda: torch.randn(rows, C, device=DEV, generator=g).to(dtype)
    rm = (torch.rand(rows, device=DEV, generator=g) > 0.2).to(torch.uint8)
    return mk(), mk(), mk(), rm


# C: 8/24/128 -> GROUP 16 (bf16/fp16 vec8); 264 -> GROUP 64; 1024 -> more
# than one in-row iteration; 33 -> scalar VEC=1; 4 -> fp32 vec4
@pytest.mark.parametrize("rows", [1, 37, 4099])
@pytest.mark.parametrize("C", [4, 8, 24, 33, 128, 264, 1024])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gatemul_fwd_bwd(ext, dtype, C, rows):
    x, g, dy, rm = _inputs(rows, C, dtype)
    for mask in (None, rm):
        tag = f"rm={mask is not None}"
        y = ext.gatemul_fwd(x, g, C, C, mask)
        dx, dg = ext.gatemul_bwd(dy, x, g, C, C, mask)
        ry, rdx, rdg = _ref(x, g, dy, mask)
        _assert_close(f"y {tag}", y, ry, dtype)
        _assert_close(f"dx {tag}", dx, rdx, dtype)
        _assert_close(f"dg {tag}", dg, rdg, dtype)
        if mask is not None:
            dead = mask == 0
            for name, t in (('y', y), ('dx', dx), ('dg', dg)):
                assert (t[dead] == 0).all(), f"{name}: masked row not 0"


# (x offset, g offset, extra row width): aligned slices; slices starting
# mid-vector; a row stride that is no multiple of 8 elements
@pytest.mark.parametrize("layout", ["aligned", "offset", "rowstride"])
@pytest.mark.parametrize("C", [8, 24, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gatemul_strided_slices(ext, dtype, C, layout):
    """hip_gatemul on channel slices of one (rows, 4C [+3]) tensor: the
    operands are read in place through their row stride and autograd
    sums dx and dg into the base tensor's gradient."""
    from alphafold2_amd.ops.hip_autograd import (_uniform_row_stride,
                                                 hip_gatemul)
    rows = 37
    ox, og, extra = {"aligned": (0, 2 * C, 0), "offset": (3, C + 5, 0),
                     "rowstride": (0, 2 * C, 3)}[layout]
    W = 4 * C + extra
    gen = torch.Generator(device=DEV).manual_seed(1)
    base0 = torch.randn(rows, W, device=DEV, generator=gen).to(dtype)
    dy = torch.randn(rows, C, device=DEV, generator=gen).to(dtype)
    rowmask = torch.rand(rows, device=DEV, generator=gen) > 0.2

    base = base0.clone().requires_grad_(True)
    x, g = base[:, ox:ox + C], base[:, og:og + C]
    assert _uniform_row_stride(x) == W and _uniform_row_stride(g) == W
    y = hip_gatemul(x, g, rowmask)
    y.backward(dy)

    ry, rdx, rdg = _ref(base0[:, ox:ox + C], base0[:, og:og + C], dy,
                        rowmask)
    rbase = torch.zeros(rows, W, device=DEV, dtype=torch.float64)
    rbase[:, ox:ox + C] = rdx
    rbase[:, og:og + C] = rdg
    _assert_close("y", y.detach(), ry, dtype)
    _assert_close("dbase", base.grad, rbase, dtype)
    assert (y.detach()[~rowmask] == 0).all()
    assert (base.grad[~rowmask] == 0).all()


@pytest.mark.parametrize("C", [8, 33])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gatemul_bwd_packed_outputs(ext, dtype, C):
    """dx_out/dg_out as slices of a NaN-filled (rows, 5C) buffer: the
    two target slices are fully overwritten with the values of the plain
    call, every other channel stays NaN."""
    rows = 37
    x, g, dy, rm = _inputs(rows, C, dtype, seed=2)
    dx, dg = ext.gatemul_bwd(dy, x, g, C, C, rm)
    buf = torch.full((rows, 5 * C), float('nan'), device=DEV, dtype=dtype)
    ext.gatemul_bwd(dy, x, g, C, C, rm, dx_out=buf[:, C:2 * C],
                    dg_out=buf[:, 3 * C:4 * C], dxs=5 * C, dgs=5 * C)
    assert torch.equal(buf[:, C:2 * C], dx)
    assert torch.equal(buf[:, 3 * C:4 * C], dg)
    assert not torch.isnan(dx).any() and not torch.isnan(dg).any()
    for lo in (0, 2 * C, 4 * C):
        assert torch.isnan(buf[:, lo:lo + C]).all(), \
            f"channels {lo}..{lo + C} were written"
    _assert_close("dx", dx, _ref(x, g, dy, rm)[1], dtype)


def test_gatemul_grid_stride_loop(ext):
    """rows = 2**20 + 37 at C = 8 (16 rows per block) is the first size
    past the 65536-block cap: the last rows are reached only through the
    grid-stride loop."""
    rows, C, dtype = 1_048_576 + 37, 8, torch.bfloat16
    x, g, dy, rm = _inputs(rows, C, dtype, seed=3)
    y = ext.gatemul_fwd(x, g, C, C, rm)
    dx, dg = ext.gatemul_bwd(dy, x, g, C, C, rm)
    ry, rdx, rdg = _ref(x, g, dy, rm)
    _assert_close("y", y, ry, dtype)
    _assert_close("dx", dx, rdx, dtype)
    _assert_close("dg", dg, rdg, dtype)
    assert (y[rm == 0] == 0).all()


def test_gatemul_rejects_mismatched_operands(ext):
    """Every operand is reinterpreted as x's dtype: each mismatch must
    raise before any launch."""
    rows, C = 16, 16
    x, g, dy, rm = _inputs(rows, C, torch.bfloat16)
    ext.gatemul_fwd(x, g, C, C, rm)                   # valid call passes
    wide = torch.zeros(rows, 2 * C, device=DEV, dtype=torch.bfloat16)
    bad_fwd = [
        lambda: ext.gatemul_fwd(x, g.float(), C, C),
        lambda: ext.gatemul_fwd(x, g.half(), C, C),
        lambda: ext.gatemul_fwd(x, g[:, :8], C, C),
        lambda: ext.gatemul_fwd(x, wide[:, ::2], C, C),
        lambda: ext.gatemul_fwd(wide[:, ::2], g, C, C),
        lambda: ext.gatemul_fwd(x, g, C, C, rm.bool()),
        lambda: ext.gatemul_fwd(x, g, C, C, rm[:-1]),
    ]
    dxo, dgo = torch.empty_like(x), torch.empty_like(x)
    bad_bwd = [
        lambda: ext.gatemul_bwd(dy.float(), x, g, C, C),
        lambda: ext.gatemul_bwd(dy, x, g.float(), C, C),
        lambda: ext.gatemul_bwd(dy, x, g, C, C, rm.float()),
        lambda: ext.gatemul_bwd(dy, x, g, C, C, rm[:-1]),
        lambda: ext.gatemul_bwd(dy, x, g, C, C, None, dx_out=dxo),
        lambda: ext.gatemul_bwd(dy, x, g, C, C, None, dg_out=dgo),
        lambda: ext.gatemul_bwd(dy, x, g, C, C, None, dx_out=dxo.float(),
                                dg_out=dgo, dxs=C, dgs=C),
        lambda: ext.gatemul_bwd(dy, x, g, C, C, None, dx_out=dxo,
                                dg_out=dgo.half(), dxs=C, dgs=C),
        lambda: ext.gatemul_bwd(dy, x, g, C, C, None, dx_out=dxo,
                                dg_out=wide[:, ::2], dxs=C, dgs=2 * C),
    ]
    for i, call in enumerate(bad_fwd + bad_bwd):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"mismatch {i} was accepted")
    torch.cuda.synchronize()


def test_softclamp_gate_mixed_dtypes_run_eager(ext):
    """An fp32 operand with bf16 gates must not reach the kernel (it
    would read the gates as fp32, past their end): the dispatcher takes
    the eager composition and matches it exactly."""
    from alphafold2_amd.ops import dispatch, eager
    gen = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(5, 37, 64, device=DEV, generator=gen)
    gates = torch.randn(5, 37, 64, device=DEV, generator=gen) \
        .to(torch.bfloat16)
    rowmask = torch.rand(5, 37, device=DEV, generator=gen) > 0.2
    want = eager.softclamp_gate(x, gates)
    assert torch.equal(dispatch.softclamp_gate(x, gates), want)
    got = dispatch.softclamp_gate(x, gates, rowmask)
    assert torch.equal(got, want * rowmask.unsqueeze(-1).to(want.dtype))
    got = dispatch.softclamp_gate(gates, x)
    assert torch.equal(got, eager.softclamp_gate(gates, x))
