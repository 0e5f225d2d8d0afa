"""GPU suite (-m gpu): results and writes of the library must not depend on where the caller's buffers sit.

Every launcher chooses a 16-byte (float4) or a scalar form from the size AND the address of every buffer of the call; the
rest of the suite reaches the scalar forms through sizes that are no multiple of 4.  Here every case runs its entry point
through the C ABI with raw pointers into one arena (tests/placement.py: 0xFF fill, each buffer at its exact size between
4 KiB guard bands, the workspace at exactly the bytes its size query returns) under these placements:

    aligned        every buffer on the 16-byte grid
    all            every data pointer of the call off the grid (fp32: +4 bytes, the byte gate `inside`: +1)
    <name>         that pointer alone off the grid -- for the fused step, which runs as forward-then-backward on the same
                   untouched workspace, this gives every mixed pair (a scalar forward with a float4 backward and the reverse);
                   `resid`, which both halves test, moves by 4 bytes (and by 8 for phase retrieval's float2 words)
    ws+4, ws-1     the workspace off the grid / one byte short of the query

and after every call checks the guards, that a successful call wrote every output element, and that a refusal wrote
nothing.  What a placement must return is decided from include/dpsx.h ("buffer placement"): success, or one of the stated
refusals -- never DPSX_EWORKSPACE for an aligned workspace of the queried size.  Results are compared with the references and
gates the suite already uses for the entry (the CPU oracle, tests/*_ref.py; test_hip_parity._fused_case's gates for the fused
step: bit-exact x0_hat and clamp gate, 1e-6 on sample, TOL = 1e-5 elsewhere; test_cg_gpu's 1e-4) and, where the header says
the forms are one body / the result is a property of the data and not of the launch, bit for bit with the aligned placement.

No case tries to make a kernel fault: every buffer lies inside one live allocation, so an overrun of the kind looked for
lands in memory this process owns and is reported by the guard check."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cg_ref
from placement import Arena, Buf, placements
from standin import rel_l2
from test_hip_parity import DEV, K, TOL, coefs_of, dev, host, make_oracle_op, make_product_op  # noqa: F401 (K: fixture)

pytestmark = pytest.mark.gpu
F32, U8, I64, I32 = torch.float32, torch.uint8, torch.int64, torch.int32
OK, EINVAL, EUNSUPPORTED, ELAUNCH, ENOMEM, EWORKSPACE = 0, -1, -2, -3, -4, -5
N, C = 2, 3
SCALE, POWER, T_STEP = 0.7, 1, 400


def _lib():
    from dps_ttc_amd import _lib as L
    return L.lib(), L


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _sync(where):
    """a device error ends the session: nothing more is started on a GPU that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after {where}: {e}", returncode=3)


def _off(b):
    """the offset a buffer takes off the 16-byte grid: one element of fp32, one byte of a byte buffer"""
    return 1 if b.dtype == U8 else 4


class Step:
    """one library call of a case.  fn(arena, ws_bytes) -> code; outs: the outputs a success writes in full;
    expect(tag, offsets) -> the code include/dpsx.h states for that placement"""

    def __init__(self, name, fn, outs, expect=None):
        self.name, self.fn, self.outs, self.expect = name, fn, tuple(outs), expect or (lambda tag, offs: OK)


def run_case(name, bufs, inputs, steps, verify, movers=None, ws=None, bitwise=(), offs_of=None, extra=(), keep=None):
    """bufs: Buf records (the workspace, if any, named `ws`, at the queried size).  inputs: {name: array} copied in after the
    fill.  movers: the buffers that take an offset (default: every fp32 / byte buffer that is no workspace).
    verify(out, tag): asserts on {name: numpy array} of every buffer after the last step.  bitwise: the outputs that
    must equal the aligned placement's bit for bit.  offs_of: {name: offset} where it is not the dtype's (`resid`: bytes
    that hold fp32 words).  extra: further (tag, offsets) placements.  keep: a dict that receives {tag: outputs}.
    Returns {tag: code of the last step run}."""
    by = {b.name: b for b in bufs}
    movers = [b.name for b in bufs if b.role != "ws" and b.dtype in (F32, U8)] if movers is None else list(movers)
    plan = placements(movers, lambda n: (offs_of or {}).get(n, _off(by[n]))) + list(extra)
    if ws is not None:
        plan += [("ws+4", {ws: 4}), ("ws-1", {})]
    codes, aligned = {}, None
    for tag, offs in plan:
        these = [Buf(b.name, (b.shape[0] - 1,), b.dtype, b.role) if (tag == "ws-1" and b.name == ws) else b for b in bufs]
        a = Arena(these, offs, DEV)
        for k, v in inputs.items():
            a.put(k, v)
        written, rc = [], OK
        for st in steps:
            before = a.snapshot()
            rc = st.fn(a, a.nbytes(ws) if ws is not None else 0)
            _sync(f"{name}: {st.name} [{tag}]")
            want = st.expect(tag, offs)
            assert rc == want, f"{name}: {st.name} [{tag}] returned {rc}, the header states {want}"
            if rc == OK:
                written += list(st.outs)
            v = a.violations(rc == OK, written=written, before=before)
            assert not v, f"{name}: {st.name} [{tag}] -> {rc}: {v}"
            if rc != OK:
                break
        codes[tag] = rc
        if rc != OK:
            continue
        out = {b.name: a.get(b.name).cpu().numpy() for b in these if b.role != "ws"}
        for k, v in inputs.items():                    # no call may write to an input that is not also an output
            if by[k].role == "in":
                assert np.array_equal(out[k].reshape(-1), np.asarray(v, dtype=out[k].dtype).reshape(-1)), \
                    f"{name} [{tag}]: input {k} changed"
        verify(out, tag)
        if tag == "aligned":
            aligned = out
        if keep is not None:
            keep[tag] = out
        for k in bitwise:
            assert np.array_equal(out[k].view(np.uint8), aligned[k].view(np.uint8)), \
                f"{name} [{tag}]: {k} differs from the aligned placement's bits"
    return codes


def ws_refused(uses_ws):
    """a workspace off the 16-byte grid or one byte short is DPSX_EWORKSPACE -- from a call that uses one"""
    return lambda tag, offs: EWORKSPACE if uses_ws and tag in ("ws+4", "ws-1") else OK


# ===================================================================== operators
# tag -> (operator of test_hip_parity.make_product_op, H, W)
OPS = {
    "gauss64": ("gauss", 64, 64),          # whole 64 x 64 tiles: the separable kernels' regular route
    "gauss48x52": ("gauss", 48, 52),       # a multiple-of-4 width off the tile grid, ks = 61
    "motion64": ("motion", 64, 64),        # the tap-list kernels' regular route
    "sr4_64": ("sr4", 64, 64),             # the row-streaming resize kernel
    "sr4_36": ("sr4", 36, 36),             # SR x4 off its fast path
    "inpaint64": ("inpaint", 64, 64),
    "denoise64": ("denoise", 64, 64),
    "denoise17": ("denoise", 17, 17),      # already scalar (867 elements): the guards and the exact-size workspace only
    "phase32": ("phase", 32, 32),          # the library transforms
    "phase256": ("phase", 256, 256),       # the hand-written spectral step
}
LINEAR = [t for t in OPS if not t.startswith("phase")]
_S = {}


def _setup(K, oracle, golden, tag, n=N):
    """operator, handle, inputs and references of one (operator, shape, n): built once, shared, never modified"""
    if (tag, n) in _S:
        return _S[(tag, n)]
    lib, L = _lib()
    name, h, w = OPS[tag]
    rng = np.random.RandomState(1000 * h + w + n)
    kernel = golden("operators")["motion.kernel"]
    mask = (np.random.RandomState(7).rand(1, 1, h, w) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=h, kernel=kernel, mask=mask)
    orc = make_oracle_op(oracle, name, hw=h, kernel=kernel, mask=mask)
    cd, ck = coefs_of(K, oracle, T_STEP)
    f = np.float32
    x_t = rng.randn(n, C, h, w).astype(f)
    target = 1.4 * np.tanh(rng.randn(n, C, h, w))
    eps = ((cd["a"] * x_t - target) / cd["b"]).astype(f)
    mo = np.concatenate([eps, rng.uniform(-1, 1, eps.shape).astype(f)], axis=1)
    noise = rng.randn(n, C, h, w).astype(f)
    y = orc.forward(rng.uniform(-1, 1, (1, C, h, w)).astype(f))
    y = (y + 0.05 * rng.randn(*y.shape)).astype(f)
    g_extra = (0.05 * rng.randn(n, C, h, w)).astype(f)
    x = rng.uniform(-1, 1, (n, C, h, w)).astype(f)
    u = rng.randn(n, *y.shape[1:]).astype(f)
    ax = orc.forward(x)
    adj = orc.adjoint(u, (h, w))                       # (phase retrieval: at x, the point of the forward just made)
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(dev(x_t))
    ws_bytes = int(lib.dpsx_op_workspace_bytes(handle._h, n, C, h, w))
    resid_bytes = int(lib.dpsx_step_resid_bytes(handle._h, n, C, h, w))
    assert ws_bytes > 0 and resid_bytes > 0
    s = SimpleNamespace(tag=tag, name=name, n=n, h=h, w=w, shape=(n, C, h, w), mshape=tuple(y.shape[1:]), op=op, fkw=fkw,
                        orc=orc, cd=cd, ck=ck, handle=handle, hp=handle._h, kind=handle.kind, ws_bytes=ws_bytes,
                        resid_bytes=resid_bytes, x_t=x_t, mo=mo, noise=noise, y=y, g_extra=g_extra, x=x, u=u, ax=ax,
                        adj=adj, refs={}, steps={}, geom=(n, C, h, w))
    _S[(tag, n)] = s
    return s


def _ws(s):
    return Buf("ws", (s.ws_bytes,), U8, "ws")


# ------------------------------------------------------------------ A and A^T
@pytest.mark.parametrize("tag", list(OPS))
def test_forward_and_adjoint(K, oracle, golden, tag):
    lib, L = _lib()
    s = _setup(K, oracle, golden, tag)
    exact = s.name in ("inpaint", "denoise")           # the suite's gate for these two is bit-exact

    def close(got, ref, what, ptag):
        if exact:
            assert np.array_equal(got, ref), (what, ptag)
        else:
            err = rel_l2(got, ref)
            assert err < TOL, (what, ptag, err)

    fwd = Step("dpsx_op_forward_f32", lambda a, wb: lib.dpsx_op_forward_f32(
        s.hp, a.ptr("x"), a.ptr("y"), *s.geom, a.ptr("ws"), wb, _stream()), ["y"], ws_refused(s.name == "phase"))
    run_case(f"{tag} forward", [Buf("x", s.shape, F32, "in"), Buf("y", (s.n,) + s.mshape, F32, "out"), _ws(s)],
             {"x": s.x}, [fwd], lambda out, ptag: close(out["y"], s.ax, "A x", ptag), ws="ws")
    adj = Step("dpsx_op_adjoint_f32", lambda a, wb: lib.dpsx_op_adjoint_f32(
        s.hp, a.ptr("u"), a.ptr("x"), a.ptr("g"), *s.geom, a.ptr("ws"), wb, _stream()), ["g"],
        ws_refused(s.name in ("gauss", "motion", "phase")))
    run_case(f"{tag} adjoint", [Buf("u", (s.n,) + s.mshape, F32, "in"), Buf("x", s.shape, F32, "in"),
                                Buf("g", s.shape, F32, "out"), _ws(s)],
             {"u": s.u, "x": s.x}, [adj], lambda out, ptag: close(out["g"], s.adj, "A^T u", ptag), ws="ws")


# ------------------------------------------------------------------ scoring
@pytest.mark.parametrize("tag", list(OPS))
def test_scoring(K, oracle, golden, tag):
    """dpsx_score_f32, dpsx_score_argmin_f32 (same costs bit for bit, torch.argmin's index) and dpsx_resample_cost_f32"""
    lib, L = _lib()
    s = _setup(K, oracle, golden, tag)
    _, ref = oracle.residual_norm(s.y, s.ax)
    prev = np.array([3.0, 0.25], dtype=np.float32)
    cur_ref, net_ref = oracle.resample_cost(s.orc, s.x, s.y, prev, "min")
    base = [Buf("x", s.shape, F32, "in"), Buf("y", (1,) + s.mshape, F32, "in"), Buf("costs", (s.n,), F32, "out")]
    costs = {}

    def check_costs(out, ptag):
        err = rel_l2(out["costs"], ref)
        assert err < TOL, (ptag, err)
        costs[ptag] = out["costs"]

    run_case(f"{tag} score", base + [_ws(s)], {"x": s.x, "y": s.y},
             [Step("dpsx_score_f32", lambda a, wb: lib.dpsx_score_f32(
                 s.hp, a.ptr("x"), a.ptr("y"), 1, a.ptr("costs"), *s.geom, a.ptr("ws"), wb, _stream()), ["costs"],
                 ws_refused(True))], check_costs, ws="ws")

    def check_select(out, ptag):
        # the same scoring launch and finisher as dpsx_score_f32 at this placement of x / y / costs
        assert np.array_equal(out["costs"], costs.get(ptag, costs["aligned"])), ptag
        b = int(out["best"][0])
        assert b == int(np.argmin(out["costs"])) and out["val"][0] == out["costs"][b], ptag

    run_case(f"{tag} score_argmin", base + [Buf("best", (1,), I64, "out"), Buf("val", (1,), F32, "out"), _ws(s)],
             {"x": s.x, "y": s.y},
             [Step("dpsx_score_argmin_f32", lambda a, wb: lib.dpsx_score_argmin_f32(
                 s.hp, a.ptr("x"), a.ptr("y"), 1, a.ptr("costs"), a.ptr("best"), a.ptr("val"), *s.geom, a.ptr("ws"), wb,
                 _stream()), ["costs", "best", "val"], ws_refused(True))], check_select, ws="ws")

    def check_cost(out, ptag):
        e1, e2 = rel_l2(out["curr"], cur_ref), rel_l2(out["net"], net_ref)
        assert e1 < TOL and e2 < TOL, (ptag, e1, e2)

    run_case(f"{tag} resample_cost",
             [Buf("x", s.shape, F32, "in"), Buf("y", (1,) + s.mshape, F32, "in"), Buf("prev", (s.n,), F32, "in"),
              Buf("curr", (s.n,), F32, "out"), Buf("net", (s.n,), F32, "out"), _ws(s)],
             {"x": s.x, "y": s.y, "prev": prev},
             [Step("dpsx_resample_cost_f32", lambda a, wb: lib.dpsx_resample_cost_f32(
                 s.hp, a.ptr("x"), a.ptr("y"), 1, a.ptr("prev"), L.POTENTIALS["min"], a.ptr("curr"), a.ptr("net"), *s.geom,
                 a.ptr("ws"), wb, _stream()), ["curr", "net"], ws_refused(True))], check_cost, ws="ws")


# ------------------------------------------------------------------ the fused step: forward, then backward
# Refusals the header states (DPSX_EUNSUPPORTED, nothing written):
#   inpainting: the step exists in its float4 form only -- any image-sized buffer of the call, or the gate, off the grid
#   phase retrieval: `resid` (the transforms' own buffer) off the grid; the spectral step (side 256) has the float4 form
#     only: forward {x_t, model_out, noise, x0_hat, sample, inside}, backward {g_model_out, g_x0_extra, inside}
#   the _rng forward: draws in its launch for 16-byte aligned buffers; blur and resize decline for others
FWD_VEC = {"inpaint": {"x_t", "model_out", "noise", "y", "x0_hat", "sample", "inside"},
           "phase256": {"x_t", "model_out", "noise", "x0_hat", "sample", "inside", "resid"},
           "phase32": {"resid"}}
BWD_VEC = {"inpaint": {"x0_hat", "y", "g_model_out", "g_extra", "inside"},
           "phase256": {"g_model_out", "g_extra", "inside", "resid"},
           "phase32": {"resid"}}
RNG_VEC = {"gauss": {"x_t", "model_out", "x0_hat", "sample", "y", "resid", "inside"},
           "motion": {"x_t", "model_out", "x0_hat", "sample", "y", "resid", "inside"},
           "sr4": {"x_t", "model_out", "x0_hat", "sample", "inside"}}


def _refusing(table, s, extra=None):
    key = s.tag if s.tag in table else s.name
    names = set(table.get(key, ())) | set((extra or {}).get(key, ()))

    def expect(tag, offs):
        if tag in ("ws+4", "ws-1"):
            return EWORKSPACE
        return EUNSUPPORTED if names & set(offs) else OK
    return expect


def _step_pair(K, oracle, s, norm_in_fwd, rng, extra):
    lib, L = _lib()
    rec = K.Rng(seed=0x5EED1234ABCD, step=T_STEP, tag=0) if rng else None
    key = (rng, extra)
    if key not in s.refs:
        noise = host(K.randn(s.shape, rec, DEV)) if rng else s.noise
        s.refs[key] = (noise, oracle.dps_step(s.orc, s.x_t, s.mo, noise, s.y, s.cd, scale=SCALE, power=POWER,
                                              g_x0_extra=s.g_extra if extra else None))
    noise, ref = s.refs[key]
    n, c, h, w = s.shape
    bufs = [Buf("x_t", s.shape, F32, "in"), Buf("model_out", (n, 2 * c, h, w), F32, "in")]
    inputs = {"x_t": s.x_t, "model_out": s.mo, "y": s.y, "g_model_out": np.zeros((n, 2 * c, h, w), dtype=np.float32)}
    if not rng:
        bufs.append(Buf("noise", s.shape, F32, "in"))
        inputs["noise"] = noise
    bufs += [Buf("y", (1,) + s.mshape, F32, "in"), Buf("x0_hat", s.shape, F32, "out"), Buf("sample", s.shape, F32, "out"),
             Buf("inside", s.shape, U8, "out"), Buf("resid", (s.resid_bytes,), U8, "ws"), Buf("norm", (n,), F32, "out"),
             Buf("g_model_out", (n, 2 * c, h, w), F32, "inout")]
    if extra:
        bufs.append(Buf("g_extra", s.shape, F32, "in"))
        inputs["g_extra"] = s.g_extra
    bufs.append(_ws(s))

    def fwd(a, wb):
        tail = (a.ptr("y"), 1, a.ptr("x0_hat"), a.ptr("sample"), a.ptr("inside"), a.ptr("resid"),
                a.ptr("norm") if norm_in_fwd else None, n, c, h, w, s.ck, a.ptr("ws"), wb, _stream())
        if rng:
            return lib.dpsx_step_fwd_rng_f32(s.hp, a.ptr("x_t"), a.ptr("model_out"), rec.rec(), *tail)
        return lib.dpsx_step_fwd_f32(s.hp, a.ptr("x_t"), a.ptr("model_out"), a.ptr("noise"), *tail)

    def bwd(a, wb):
        head = (s.hp, a.ptr("resid"), a.ptr("norm") if norm_in_fwd else None, None if norm_in_fwd else a.ptr("norm"),
                a.ptr("inside"), a.ptr("x0_hat"), a.ptr("y"), 1, SCALE, POWER)
        tail = (a.ptr("g_model_out"), n, c, h, w, s.ck, a.ptr("ws"), wb, _stream())
        if extra:
            return lib.dpsx_step_bwd_extra_f32(*head, a.ptr("g_extra"), *tail)
        return lib.dpsx_step_bwd_f32(*head, *tail)

    def verify(out, ptag):
        np.testing.assert_array_equal(out["x0_hat"], ref["x0_hat"], err_msg=ptag)
        np.testing.assert_array_equal(out["inside"], ref["inside"], err_msg=ptag)
        errs = {"sample": rel_l2(out["sample"], ref["sample"]), "norm": rel_l2(out["norm"], ref["norm"]),
                "g_model_out": rel_l2(out["g_model_out"], ref["g_model_out"])}
        assert errs["sample"] < 1e-6 and errs["norm"] < TOL and errs["g_model_out"] < TOL, (ptag, errs)
        assert np.all(out["g_model_out"][:, c:] == 0), ptag
        if s.name == "inpaint":
            np.testing.assert_array_equal(out["g_model_out"][:, :c] != 0, ref["g_model_out"][:, :c] != 0, err_msg=ptag)

    outs_f = ["x0_hat", "sample", "inside"] + (["norm"] if norm_in_fwd else [])
    steps = [Step("dpsx_step_fwd_rng_f32" if rng else "dpsx_step_fwd_f32", fwd, outs_f,
                  _refusing(FWD_VEC, s, RNG_VEC if rng else None)),
             Step("dpsx_step_bwd_extra_f32" if extra else "dpsx_step_bwd_f32", bwd, [] if norm_in_fwd else ["norm"],
                  _refusing(BWD_VEC, s))]
    # `resid` carries fp32 words (blur, resize, identity: the residual; phase: float2 words, hence +8 as well) and is the one
    # buffer both halves test: it moves like the fp32 buffers
    movers = [b.name for b in bufs if b.name == "resid" or (b.role != "ws" and b.dtype in (F32, U8))]
    kept = s.steps.setdefault((norm_in_fwd, rng, extra), {})
    codes = run_case(f"{s.tag} step norm_in_fwd={norm_in_fwd} rng={rng} extra={extra}", bufs, inputs, steps, verify,
                     movers=movers, ws="ws", offs_of={"resid": 4},
                     extra=[("resid+8", {"resid": 8})] if s.name == "phase" else [], keep=kept,
                     bitwise=("x0_hat", "inside", "sample"))       # S1 is one expression per element in every form
    assert codes["resid"] == (EUNSUPPORTED if s.name == "phase" or (rng and s.name in ("gauss", "motion")) else OK)
    return codes


@pytest.mark.parametrize("tag", list(OPS))
def test_fused_step_norm_in_backward(K, oracle, golden, tag):
    """dpsx_step_fwd_f32 with norm == NULL, then dpsx_step_bwd_f32 finalising the partials left in the workspace"""
    s = _setup(K, oracle, golden, tag)
    codes = _step_pair(K, oracle, s, norm_in_fwd=False, rng=False, extra=False)
    assert codes["aligned"] == OK


@pytest.mark.parametrize("tag", list(OPS))
def test_fused_step_norm_in_forward_extra_cotangent(K, oracle, golden, tag):
    """dpsx_step_fwd_f32 with norm != NULL (the in-launch finisher), then dpsx_step_bwd_extra_f32"""
    s = _setup(K, oracle, golden, tag)
    codes = _step_pair(K, oracle, s, norm_in_fwd=True, rng=False, extra=True)
    assert codes["aligned"] == OK
    # the in-launch finisher re-sums the partials in k_finalize_norm's / the backward prologue's order: the same bits as the
    # pair that leaves the norm to the backward half, placement by placement
    if (False, False, False) not in s.steps:
        _step_pair(K, oracle, s, norm_in_fwd=False, rng=False, extra=False)
    late, early = s.steps[(False, False, False)], s.steps[(True, False, True)]
    if s.name == "phase":          # (no in-launch finisher there: dpsx_step_fwd_f32 ends with k_finalize_norm itself)
        return
    shared = [t for t in early if t in late]
    assert "aligned" in shared and "resid" in shared          # (inpainting refuses the other placements)
    for t in shared:
        assert np.array_equal(early[t]["norm"].view(np.uint32), late[t]["norm"].view(np.uint32)), (tag, t)


@pytest.mark.parametrize("tag", list(OPS))
def test_fused_step_in_kernel_draw(K, oracle, golden, tag):
    """dpsx_step_fwd_rng_f32 where dpsx_step_draws_in_kernel is 1 (elsewhere: the stated refusal, nothing written)"""
    lib, L = _lib()
    s = _setup(K, oracle, golden, tag)
    n, c, h, w = s.shape
    if not lib.dpsx_step_draws_in_kernel(s.hp, c, h, w):
        a = Arena([Buf("x", s.shape, F32, "out"), Buf("b", s.shape, U8, "out"), Buf("r", (s.resid_bytes,), U8, "ws"),
                   _ws(s)], {}, DEV)
        before = a.snapshot()
        rec = K.Rng(seed=1, step=2)
        rc = lib.dpsx_step_fwd_rng_f32(s.hp, a.ptr("x"), a.ptr("x"), rec.rec(), a.ptr("x"), 1, a.ptr("x"), a.ptr("x"),
                                       a.ptr("b"), a.ptr("r"), None, n, c, h, w, s.ck, a.ptr("ws"), s.ws_bytes, _stream())
        torch.cuda.synchronize()
        assert rc == EUNSUPPORTED and not a.violations(False, before=before)
        return
    codes = _step_pair(K, oracle, s, norm_in_fwd=False, rng=True, extra=False)
    assert codes["aligned"] == OK


@pytest.mark.parametrize("tag", ["phase32", "phase256"])
def test_phase_backward_refuses_an_unaligned_resid(K, oracle, golden, tag):
    """The forward half refuses `resid` off the 16-byte grid, so the pair above never reaches the backward half's own
    refusal: here the forward runs aligned and the backward is handed the same buffer 4 and 8 bytes further on (inside
    the buffer: nothing is launched, nothing read)"""
    import ctypes
    lib, L = _lib()
    s = _setup(K, oracle, golden, tag)
    n, c, h, w = s.shape
    a = Arena([Buf("x_t", s.shape, F32, "in"), Buf("model_out", (n, 2 * c, h, w), F32, "in"), Buf("noise", s.shape, F32, "in"),
               Buf("y", (1,) + s.mshape, F32, "in"), Buf("x0_hat", s.shape, F32, "out"), Buf("sample", s.shape, F32, "out"),
               Buf("inside", s.shape, U8, "out"), Buf("resid", (s.resid_bytes,), U8, "ws"), Buf("norm", (n,), F32, "out"),
               Buf("g_model_out", (n, 2 * c, h, w), F32, "inout"), _ws(s)], {}, DEV)
    for k, v in (("x_t", s.x_t), ("model_out", s.mo), ("noise", s.noise), ("y", s.y),
                 ("g_model_out", np.zeros((n, 2 * c, h, w), dtype=np.float32))):
        a.put(k, v)
    rc = lib.dpsx_step_fwd_f32(s.hp, a.ptr("x_t"), a.ptr("model_out"), a.ptr("noise"), a.ptr("y"), 1, a.ptr("x0_hat"),
                               a.ptr("sample"), a.ptr("inside"), a.ptr("resid"), None, n, c, h, w, s.ck, a.ptr("ws"),
                               s.ws_bytes, _stream())
    _sync(f"{tag} forward")
    assert rc == OK and not a.violations(True, written=["x0_hat", "sample", "inside"])
    for off in (4, 8):
        before = a.snapshot()
        rc = lib.dpsx_step_bwd_f32(s.hp, ctypes.c_void_p(a.addr("resid") + off), None, a.ptr("norm"), a.ptr("inside"),
                                   a.ptr("x0_hat"), a.ptr("y"), 1, SCALE, POWER, a.ptr("g_model_out"), n, c, h, w, s.ck,
                                   a.ptr("ws"), s.ws_bytes, _stream())
        _sync(f"{tag} backward, resid + {off}")
        assert rc == EUNSUPPORTED, (off, rc)
        assert not a.violations(False, before=before), off


# ------------------------------------------------------------------ the search steps
def _search(K, oracle, golden, tag, form):
    """form: 'seg' (a state per particle), 'one_seg' (a state per image), 'beam' (the two best of each image)"""
    lib, L = _lib()
    n, segs = 4, 2
    s = _setup(K, oracle, golden, tag, n=n)
    _, c, h, w = s.shape
    states = {"seg": n, "one_seg": segs, "beam": n}[form]
    keep = {"seg": n, "one_seg": segs, "beam": n}[form]          # rows of x_next
    picks = {"seg": segs, "one_seg": segs, "beam": n}[form]      # entries of best / val
    x_t, mo = s.x_t[:states], s.mo[:states]
    rows = np.arange(n) // (n // states)
    if form not in s.refs:
        s.refs[form] = oracle.posterior_fwd(x_t[rows], mo[rows], s.noise, s.cd)["sample"]
    sample_ref = s.refs[form]
    bufs = [Buf("x_t", (states, c, h, w), F32, "in"), Buf("model_out", (states, 2 * c, h, w), F32, "in"),
            Buf("noise", s.shape, F32, "in"), Buf("y", (1,) + s.mshape, F32, "in"), Buf("sample", s.shape, F32, "out"),
            Buf("costs", (n,), F32, "out"), Buf("best", (picks,), I64, "out"), Buf("val", (picks,), F32, "out"),
            Buf("x_next", (keep, c, h, w), F32, "out"), _ws(s)]

    def call(a, wb):
        head = (s.hp, a.ptr("x_t"), a.ptr("model_out"), a.ptr("noise"))
        mid = (a.ptr("y"), 1, a.ptr("sample"), a.ptr("costs"), a.ptr("best"), a.ptr("val"), a.ptr("x_next"), segs)
        tail = (n, c, h, w, s.ck, a.ptr("ws"), wb, _stream())
        if form == "seg":
            return lib.dpsx_search_step_seg_f32(*head, *mid, *tail)
        if form == "one_seg":
            return lib.dpsx_search_step_one_seg_f32(*head, *mid, *tail)
        return lib.dpsx_search_step_beam_f32(*head, None, *mid, states, 2, *tail)

    def verify(out, ptag):
        assert rel_l2(out["sample"], sample_ref) < 1e-6, ptag
        _, cref = oracle.residual_norm(s.y, s.orc.forward(out["sample"]))     # of the device's own proposals
        err = rel_l2(out["costs"], cref)
        assert err < TOL, (ptag, err)
        k = n // segs
        for m in range(segs):
            seg = out["costs"][m * k:(m + 1) * k]
            if form == "beam":
                order = m * k + np.argsort(seg, kind="stable")
                assert out["best"][2 * m:2 * m + 2].tolist() == order[:2].tolist(), (ptag, m)
                assert np.array_equal(out["x_next"][2 * m:2 * m + 2], out["sample"][order[:2]]), (ptag, m)
                assert np.array_equal(out["val"][2 * m:2 * m + 2], out["costs"][order[:2]]), (ptag, m)
                continue
            b = m * k + int(np.argmin(seg))
            assert int(out["best"][m]) == b and out["val"][m] == out["costs"][b], (ptag, m)
            want = out["sample"][b]
            got = out["x_next"][m * k:(m + 1) * k] if form == "seg" else out["x_next"][m:m + 1]
            assert all(np.array_equal(g, want) for g in got), (ptag, m)

    name = {"seg": "dpsx_search_step_seg_f32", "one_seg": "dpsx_search_step_one_seg_f32",
            "beam": "dpsx_search_step_beam_f32"}[form]
    run_case(f"{tag} {name}", bufs, {"x_t": x_t, "model_out": mo, "noise": s.noise, "y": s.y},
             [Step(name, call, ["sample", "costs", "best", "val", "x_next"], ws_refused(True))], verify, ws="ws",
             bitwise=("sample",))          # S1's forms are one body (particle_pass.h)


SEARCH_OPS = list(OPS)


@pytest.mark.parametrize("tag", SEARCH_OPS)
def test_search_step_seg(K, oracle, golden, tag):
    _search(K, oracle, golden, tag, "seg")


@pytest.mark.parametrize("tag", SEARCH_OPS)
def test_search_step_one_seg(K, oracle, golden, tag):
    _search(K, oracle, golden, tag, "one_seg")


@pytest.mark.parametrize("tag", SEARCH_OPS)
def test_search_step_beam(K, oracle, golden, tag):
    _search(K, oracle, golden, tag, "beam")


# ------------------------------------------------------------------ the CG step
@pytest.mark.parametrize("tag", LINEAR)
def test_cg_step(K, oracle, golden, tag):
    lib, L = _lib()
    s = _setup(K, oracle, golden, tag)
    n, c, h, w = s.shape
    rho, iters = 0.25, 3
    need = int(lib.dpsx_cg_workspace_bytes(s.hp, n, c, h, w))
    assert need > 0
    x0 = np.clip(s.x + 0.3 * s.g_extra * 20, -1, 1).astype(np.float32)
    d_ref, dist_ref = cg_ref.solve(s.orc, x0, s.y, rho, iters)
    kappa = float(cg_ref.kappa(s.cd))
    x_ref = s.noise.astype(np.float64) + kappa * d_ref
    bufs = [Buf("x0_hat", s.shape, F32, "in"), Buf("sample", s.shape, F32, "in"), Buf("y", (1,) + s.mshape, F32, "in"),
            Buf("x_next", s.shape, F32, "out"), Buf("dist", (n,), F32, "out"), Buf("d", s.shape, F32, "out"),
            Buf("ws", (need,), U8, "ws")]

    def verify(out, ptag):
        errs = rel_l2(out["d"], d_ref), rel_l2(out["x_next"], x_ref), rel_l2(out["dist"], dist_ref)
        assert max(errs) <= 1e-4, (ptag, errs)
        assert np.array_equal(out["x_next"], s.noise + np.float32(kappa) * out["d"]), ptag

    run_case(f"{tag} cg", bufs, {"x0_hat": x0, "sample": s.noise, "y": s.y},
             [Step("dpsx_cg_step_f32", lambda a, wb: lib.dpsx_cg_step_f32(
                 s.hp, a.ptr("x0_hat"), a.ptr("sample"), a.ptr("y"), 1, rho, iters, s.ck, a.ptr("x_next"), a.ptr("dist"),
                 a.ptr("d"), n, c, h, w, a.ptr("ws"), wb, _stream()), ["x_next", "dist", "d"], ws_refused(True))],
             verify, ws="ws")


def test_the_separable_adjoint_runs_in_the_queried_workspace(K, oracle, golden):
    """The finding this suite started from: dpsx_op_workspace_bytes gave a separable kernel no adjoint scratch at shapes
    whose float4 path needs none, and one pointer off the grid sent the same shape through the two-launch adjoint, which
    then answered DPSX_EWORKSPACE to a workspace of exactly the queried size.  The query knows no pointer: it covers every
    placement, for separable kernels as for tap lists."""
    lib, L = _lib()
    for tag in ("gauss64", "gauss48x52"):
        s = _setup(K, oracle, golden, tag)
        n, c, h, w = s.shape
        assert s.kind == L.KIND_SEP
        assert s.ws_bytes > n * c * h * w * 4                      # the padded domain of every plane, beside the partials
        a = Arena([Buf("u", s.shape, F32, "in"), Buf("g", s.shape, F32, "out"), _ws(s)], {"u": 4}, DEV)
        a.put("u", s.u)
        rc = lib.dpsx_op_adjoint_f32(s.hp, a.ptr("u"), None, a.ptr("g"), n, c, h, w, a.ptr("ws"), s.ws_bytes, _stream())
        torch.cuda.synchronize()
        assert rc == OK, rc
        assert not a.violations(True, written=["g"])


# ===================================================================== particle passes
# N = 3 particles; 3 x 16 x 16 (768 elements: whole float4 units, more than one block) and 1 x 5 x 4 (20 elements: one
# ragged block).  Element-wise outputs, integer results and the norm finisher are the aligned placement's bit for bit (one
# body, two unit widths); sums whose order the unit width changes (the corr partials, the DSG sums and what follows from
# them) are held to their restatements under the bounds of test_smc_gpu.py / test_dsg_gpu.py.
PN = 3
PSHAPES = {"3x16x16": (3, 16, 16), "1x5x4": (1, 5, 4)}
T_PART = 700
_P = {}


def _particles(K, oracle, key):
    if key in _P:
        return _P[key]
    c, h, w = PSHAPES[key]
    rng = np.random.RandomState(17 + h)
    f = np.float32
    cd, ck = coefs_of(K, oracle, T_PART)
    shape = (PN, c, h, w)
    p = SimpleNamespace(shape=shape, c=c, chw=c * h * w, cd=cd, ck=ck, x=rng.randn(*shape).astype(f),
                        mo=rng.randn(PN, 2 * c, h, w).astype(f) * f(0.5), z=rng.randn(*shape).astype(f),
                        g0=rng.randn(*shape).astype(f), g1=rng.randn(*shape).astype(f),
                        g_mo=np.concatenate([rng.randn(*shape).astype(f) * f(0.1), np.zeros(shape, f)], axis=1),
                        g_unet=(1e-2 * rng.randn(*shape)).astype(f), sample=rng.randn(*shape).astype(f),
                        rec=K.Rng(seed=(3 << 32) + 99, step=T_PART, tag=0, particle_base=5))
    _P[key] = p
    return p


def _one(name, fn, bufs, inputs, outs, verify, bitwise=None, movers=None):
    """a case of one call that succeeds at every placement"""
    bufs = list(bufs)
    movers = [b.name for b in bufs if b.role != "ws" and b.dtype in (F32, U8, I32)] if movers is None else movers
    return run_case(name, bufs, inputs, [Step(name, lambda a, wb: fn(a), outs)], verify, movers=movers,
                    bitwise=tuple(outs) if bitwise is None else bitwise)


@pytest.mark.parametrize("key", list(PSHAPES))
def test_posterior_step(K, oracle, key):
    """dpsx_posterior_fwd_f32, its _rng form and dpsx_posterior_bwd_f32"""
    lib, L = _lib()
    p = _particles(K, oracle, key)
    n, c, h, w = p.shape
    io = [Buf("x0_hat", p.shape, F32, "out"), Buf("sample", p.shape, F32, "out"), Buf("inside", p.shape, U8, "out")]
    for rng in (False, True):
        z = host(K.randn(p.shape, p.rec, DEV)) if rng else p.z
        ref = oracle.posterior_fwd(p.x, p.mo, z, p.cd)

        def verify(out, ptag, ref=ref):
            np.testing.assert_array_equal(out["x0_hat"], ref["x0_hat"], err_msg=ptag)
            np.testing.assert_array_equal(out["inside"], ref["inside"], err_msg=ptag)
            assert rel_l2(out["sample"], ref["sample"]) < 1e-6, ptag

        bufs = [Buf("x_t", p.shape, F32, "in"), Buf("model_out", (n, 2 * c, h, w), F32, "in")]
        if rng:
            _one("dpsx_posterior_fwd_rng_f32", lambda a: lib.dpsx_posterior_fwd_rng_f32(
                a.ptr("x_t"), a.ptr("model_out"), p.rec.rec(), a.ptr("x0_hat"), a.ptr("sample"), a.ptr("inside"), n, p.chw,
                p.ck, _stream()), bufs + io, {"x_t": p.x, "model_out": p.mo}, ["x0_hat", "sample", "inside"], verify)
        else:
            _one("dpsx_posterior_fwd_f32", lambda a: lib.dpsx_posterior_fwd_f32(
                a.ptr("x_t"), a.ptr("model_out"), a.ptr("noise"), a.ptr("x0_hat"), a.ptr("sample"), a.ptr("inside"), n,
                p.chw, p.ck, _stream()), bufs + [Buf("noise", p.shape, F32, "in")] + io,
                {"x_t": p.x, "model_out": p.mo, "noise": p.z}, ["x0_hat", "sample", "inside"], verify)
    gx_ref, gmo_ref = oracle.posterior_bwd(p.g0, p.g1, p.x, p.mo, p.z, p.cd)

    def verify_bwd(out, ptag):
        e1, e2 = rel_l2(out["g_x"], gx_ref), rel_l2(out["g_mo"], gmo_ref)
        assert e1 < TOL and e2 < TOL, (ptag, e1, e2)

    _one("dpsx_posterior_bwd_f32", lambda a: lib.dpsx_posterior_bwd_f32(
        a.ptr("g_x0"), a.ptr("g_sample"), a.ptr("x_t"), a.ptr("model_out"), a.ptr("noise"), a.ptr("g_x"), a.ptr("g_mo"), n,
        p.chw, p.ck, _stream()),
        [Buf("g_x0", p.shape, F32, "in"), Buf("g_sample", p.shape, F32, "in"), Buf("x_t", p.shape, F32, "in"),
         Buf("model_out", (n, 2 * c, h, w), F32, "in"), Buf("noise", p.shape, F32, "in"), Buf("g_x", p.shape, F32, "out"),
         Buf("g_mo", (n, 2 * c, h, w), F32, "out")],
        {"g_x0": p.g0, "g_sample": p.g1, "x_t": p.x, "model_out": p.mo, "noise": p.z}, ["g_x", "g_mo"], verify_bwd)


@pytest.mark.parametrize("key", list(PSHAPES))
def test_randn_with_bits(K, oracle, key):
    import noise_ref
    from test_noise_device_gpu import BOUND
    lib, L = _lib()
    p = _particles(K, oracle, key)
    words = 4 * ((p.chw + 3) // 4)
    ref_bits = noise_ref.bits(PN, p.chw, p.rec.seed, p.rec.step, p.rec.tag, p.rec.particle_base, p.rec.per_image)
    ref = noise_ref.normals_from_bits(ref_bits, p.chw)

    def verify(out, ptag):
        assert np.array_equal(out["bits"].view(np.uint32), ref_bits), ptag
        assert float(np.abs(out["out"].astype(np.float64) - ref).max()) <= BOUND, ptag

    _one("dpsx_randn_f32", lambda a: lib.dpsx_randn_f32(a.ptr("out"), a.ptr("bits"), PN, p.chw, p.rec.rec(), _stream()),
         [Buf("out", (PN, p.chw), F32, "out"), Buf("bits", (PN, words), I32, "out")], {}, ["out", "bits"], verify)


@pytest.mark.parametrize("key", list(PSHAPES))
def test_updates(K, oracle, key):
    """dpsx_step_update_f32, dpsx_update_f32, dpsx_step_update_corr_f32, dpsx_step_update_dsg_f32, dpsx_smc_accum_f32"""
    import dsg_ref
    import smc_ref
    lib, L = _lib()
    p = _particles(K, oracle, key)
    n, c, h, w = p.shape
    slots = int(lib.dpsx_corr_slots(p.chw))
    s = smc_ref.update(p.g_mo[:, :c], p.g_unet, p.ck)
    x_ref = p.sample.astype(np.float64) - s
    common = [Buf("sample", p.shape, F32, "in"), Buf("g_mo", (n, 2 * c, h, w), F32, "in"), Buf("g_unet", p.shape, F32, "in")]
    cin = {"sample": p.sample, "g_mo": p.g_mo, "g_unet": p.g_unet}
    kept = {}

    def verify_x(out, ptag):
        assert rel_l2(out["x_next"], x_ref) < 1e-6, ptag
        kept.setdefault("x_next", out["x_next"])

    _one("dpsx_step_update_f32", lambda a: lib.dpsx_step_update_f32(
        a.ptr("sample"), a.ptr("g_mo"), a.ptr("g_unet"), a.ptr("x_next"), n, p.chw, p.ck, _stream()),
        common + [Buf("x_next", p.shape, F32, "out")], cin, ["x_next"], verify_x)

    def verify_plain(out, ptag):
        assert rel_l2(out["out"], p.sample.astype(np.float64) - (p.g0.astype(np.float64) + p.g1)) < 1e-6, ptag

    _one("dpsx_update_f32", lambda a: lib.dpsx_update_f32(
        a.ptr("sample"), a.ptr("g_a"), a.ptr("g_b"), a.ptr("out"), n * p.chw, _stream()),
        [Buf("sample", p.shape, F32, "in"), Buf("g_a", p.shape, F32, "in"), Buf("g_b", p.shape, F32, "in"),
         Buf("out", p.shape, F32, "out")], {"sample": p.sample, "g_a": p.g0, "g_b": p.g1}, ["out"], verify_plain)

    noisy = common + [Buf("model_out", (n, 2 * c, h, w), F32, "in"), Buf("noise", p.shape, F32, "in"),
                      Buf("x_next", p.shape, F32, "out")]
    nin = dict(cin, model_out=p.mo, noise=p.z)
    corr_ref, scale = smc_ref.correction(p.g_mo[:, :c], p.g_unet, p.mo[:, c:], p.z, p.ck)

    def verify_corr(out, ptag):
        assert np.array_equal(out["x_next"], kept["x_next"]), ptag            # dpsx_step_update_f32's bits (the header)
        got = out["corr"].astype(np.float64).sum(axis=1)
        assert np.all(np.abs(got - corr_ref) <= 1e-5 * scale), (ptag, got, corr_ref)

    _one("dpsx_step_update_corr_f32", lambda a: lib.dpsx_step_update_corr_f32(
        a.ptr("sample"), a.ptr("g_mo"), a.ptr("g_unet"), a.ptr("model_out"), a.ptr("noise"), None, a.ptr("x_next"),
        a.ptr("corr"), n, p.chw, p.ck, _stream()), noisy + [Buf("corr", (n, slots), F32, "out")], nin, ["x_next", "corr"],
        verify_corr, bitwise=("x_next",))

    rate = 0.5
    ref = dsg_ref.restate(p.sample, p.g_mo[:, :c], p.g_unet, p.mo[:, c:], p.z, p.ck, rate)
    flat = lambda a: np.sqrt((a.reshape(n, -1) ** 2).sum(axis=1))

    def verify_dsg(out, ptag):
        got = out["stats"].astype(np.float64).sum(axis=1)
        for j, nm in enumerate(("S", "Nn", "C", "R")):
            assert np.all(np.abs(got[:, j] - ref[nm]) <= 1e-5 * ref["mag"][nm]), (ptag, nm)
        D = out["x_next"].astype(np.float64) - (p.sample.astype(np.float64) - ref["n"])
        assert np.all(flat(D - ref["D"]) / flat(ref["D"]) <= 1e-4), ptag

    _one("dpsx_step_update_dsg_f32", lambda a: lib.dpsx_step_update_dsg_f32(
        a.ptr("sample"), a.ptr("g_mo"), a.ptr("g_unet"), a.ptr("model_out"), a.ptr("noise"), None, rate, a.ptr("x_next"),
        a.ptr("stats"), n, p.chw, p.ck, _stream()), noisy + [Buf("stats", (n, slots, 4), F32, "out")], nin,
        ["x_next", "stats"], verify_dsg, bitwise=())

    rng = np.random.RandomState(5)
    E0, dp0 = rng.randn(n).astype(np.float32), (40 + rng.randn(n)).astype(np.float32)
    dc, part = (50 + 10 * rng.randn(n)).astype(np.float32), (3 * rng.randn(n, slots)).astype(np.float32)
    reset = np.array([0], dtype=np.uint8)
    E_ref, dp_ref, mag = smc_ref.accum(E0, dp0, dc, part, reset, 1, 0.37, 2, 0.25)

    def verify_acc(out, ptag):
        err = np.abs(out["E"].astype(np.float64) - E_ref.astype(np.float64))
        assert np.all(err <= np.maximum(2 * np.spacing(np.abs(E_ref)).astype(np.float64), 1e-6 * mag)), ptag
        assert np.array_equal(out["d_prev"], dc), ptag

    _one("dpsx_smc_accum_f32", lambda a: lib.dpsx_smc_accum_f32(
        a.ptr("E"), a.ptr("d_prev"), a.ptr("d_cur"), a.ptr("part"), slots, a.ptr("reset"), 1, n, 0.37, 2, 0.25, _stream()),
        [Buf("E", (n,), F32, "inout"), Buf("d_prev", (n,), F32, "inout"), Buf("d_cur", (n,), F32, "in"),
         Buf("part", (n, slots), F32, "in"), Buf("reset", (1,), U8, "in")],
        {"E": E0, "d_prev": dp0, "d_cur": dc, "part": part, "reset": reset}, [], verify_acc, bitwise=("E", "d_prev"))


@pytest.mark.parametrize("key", list(PSHAPES))
def test_residual_norm_and_its_vjp(K, oracle, key):
    lib, L = _lib()
    p = _particles(K, oracle, key)
    n, m = PN, p.chw
    y, ax = p.sample[:1], p.x
    r_ref, n_ref = oracle.residual_norm(y, ax)

    def verify(out, ptag):
        np.testing.assert_array_equal(out["r"], r_ref, err_msg=ptag)
        assert rel_l2(out["norm"], n_ref) < 1e-6, ptag

    # no size query: the header's formula, min(256, max(1, ceil(m / 4096))) fp32 partial sums per particle -- 12 bytes
    # here; 4-byte alignment suffices (plain fp32 words), one byte short is refused
    parts = min(256, max(1, (m + 4095) // 4096))
    rbufs = [Buf("y", (1,) + p.shape[1:], F32, "in"), Buf("ax", p.shape, F32, "in"), Buf("r", p.shape, F32, "out"),
             Buf("norm", (n,), F32, "out"), Buf("ws", (n * parts * 4,), U8, "ws")]
    run_case("dpsx_residual_norm_f32", rbufs, {"y": y, "ax": ax},
             [Step("dpsx_residual_norm_f32", lambda a, wb: lib.dpsx_residual_norm_f32(
                 a.ptr("y"), 1, a.ptr("ax"), a.ptr("r"), a.ptr("norm"), n, m, a.ptr("ws"), wb, _stream()), ["r", "norm"],
                 lambda tag, offs: EWORKSPACE if tag == "ws-1" else OK)], verify, ws="ws", bitwise=("r", "norm"))
    gn = np.array([0.3, 1.0, 2.5], dtype=np.float32)
    for power in (1, 2):
        g_ref = oracle.norm_bwd(r_ref, n_ref, gn, power)
        _one("dpsx_norm_bwd_f32", lambda a: lib.dpsx_norm_bwd_f32(
            a.ptr("r"), a.ptr("norm"), a.ptr("g_norm"), power, a.ptr("g_ax"), n, m, _stream()),
            [Buf("r", p.shape, F32, "in"), Buf("norm", (n,), F32, "in"), Buf("g_norm", (n,), F32, "in"),
             Buf("g_ax", p.shape, F32, "out")], {"r": r_ref, "norm": n_ref, "g_norm": gn}, ["g_ax"],
            lambda out, ptag: rel_l2(out["g_ax"], g_ref) < 1e-6 or pytest.fail(f"norm_bwd {ptag}"))


@pytest.mark.parametrize("key", list(PSHAPES))
def test_gather_and_replicate(K, oracle, key):
    lib, L = _lib()
    p = _particles(K, oracle, key)
    src = p.x.reshape(PN, p.chw)
    ids = np.array([2, 0, 2, 1], dtype=np.int64)
    _one("dpsx_gather_f32", lambda a: lib.dpsx_gather_f32(a.ptr("src"), a.ptr("ids"), a.ptr("dst"), 4, PN, p.chw, _stream()),
         [Buf("src", (PN, p.chw), F32, "in"), Buf("ids", (4,), I64, "in"), Buf("dst", (4, p.chw), F32, "out")],
         {"src": src, "ids": ids}, ["dst"], lambda out, ptag: np.testing.assert_array_equal(out["dst"], src[ids], err_msg=ptag))
    idx = np.array([1], dtype=np.int64)
    _one("dpsx_replicate_f32", lambda a: lib.dpsx_replicate_f32(a.ptr("src"), a.ptr("idx"), a.ptr("dst"), 5, PN, p.chw, _stream()),
         [Buf("src", (PN, p.chw), F32, "in"), Buf("idx", (1,), I64, "in"), Buf("dst", (5, p.chw), F32, "out")],
         {"src": src, "idx": idx}, ["dst"],
         lambda out, ptag: np.testing.assert_array_equal(out["dst"], np.repeat(src[1:2], 5, axis=0), err_msg=ptag))


def test_selects():
    """dpsx_argmin_f32, dpsx_argmin_seg_f32, dpsx_topk_seg_f32 (vectors of costs: the guards and the unaligned vector)"""
    import beam_ref
    lib, L = _lib()
    v = np.array([3.0, 0.5, 2.0, 0.5, 7.0, 1.0], dtype=np.float32)

    def check(want):
        def verify(out, ptag):
            assert out["idx"].tolist() == list(want), ptag
            assert np.array_equal(out["val"], v[list(want)]), ptag
        return verify

    def bufs(k):
        return [Buf("v", (6,), F32, "in"), Buf("idx", (k,), I64, "out"), Buf("val", (k,), F32, "out")]

    _one("dpsx_argmin_f32", lambda a: lib.dpsx_argmin_f32(a.ptr("v"), 6, a.ptr("idx"), a.ptr("val"), _stream()),
         bufs(1), {"v": v}, ["idx", "val"], check([1]))
    _one("dpsx_argmin_seg_f32", lambda a: lib.dpsx_argmin_seg_f32(a.ptr("v"), 2, 3, a.ptr("idx"), a.ptr("val"), _stream()),
         bufs(2), {"v": v}, ["idx", "val"], check(beam_ref.topb(v, 2, 1)))
    _one("dpsx_topk_seg_f32", lambda a: lib.dpsx_topk_seg_f32(a.ptr("v"), 2, 3, 2, a.ptr("idx"), a.ptr("val"), _stream()),
         bufs(4), {"v": v}, ["idx", "val"], check(beam_ref.topb(v, 2, 2)))


@pytest.mark.parametrize("key", list(PSHAPES))
def test_resampling(K, oracle, key):
    """dpsx_resample_draw_seg_f32 / _ex and dpsx_resample_seg_f32 / _ex: one segment of three particles"""
    import resample_ref
    import resample_scheme_ref as S
    lib, L = _lib()
    p = _particles(K, oracle, key)
    n, chw = PN, p.chw
    src = p.x.reshape(n, chw)
    d = np.array([4.0, 1.0, 2.5], dtype=np.float32)
    u = np.array([0.05, 0.5, 0.93], dtype=np.float32)
    inv = 0.75
    q_ref = resample_ref.weights(d, np.float32(inv))
    draw = [Buf("d", (n,), F32, "in"), Buf("u", (n,), F32, "in"), Buf("ids", (n,), I64, "out"), Buf("q", (n,), I32, "out")]
    moved = [Buf("src", (n, chw), F32, "in"), Buf("dst", (n, chw), F32, "out"), Buf("d_out", (n,), F32, "out")]
    diag = [Buf("flag", (1,), U8, "out"), Buf("ess", (1,), F32, "out")]

    def verify(scheme, ess_q16, gathers, ex):
        def f(out, ptag):
            q = out["q"].astype(np.int64)
            assert np.abs(q - q_ref).max() <= 6, ptag                  # the device's expf (test_resample_device_gpu's gate)
            ids, flags, ess = S.draw_segments(q, u, 1, scheme, ess_q16)
            assert np.array_equal(out["ids"], ids), ptag               # integer arithmetic from q on: exact
            if gathers:
                assert np.array_equal(out["dst"], src[ids]) and np.array_equal(out["d_out"], d[ids]), ptag
            if ex:
                assert np.array_equal(out["flag"], flags) and np.array_equal(out["ess"], ess), ptag
        return f

    _one("dpsx_resample_draw_seg_f32", lambda a: lib.dpsx_resample_draw_seg_f32(
        a.ptr("d"), a.ptr("u"), 1, n, inv, a.ptr("ids"), a.ptr("q"), _stream()), draw, {"d": d, "u": u}, ["ids", "q"],
        verify(S.MULTINOMIAL, S.ONE_Q16, False, False))
    _one("dpsx_resample_seg_f32", lambda a: lib.dpsx_resample_seg_f32(
        a.ptr("d"), a.ptr("u"), 1, n, inv, a.ptr("src"), a.ptr("dst"), a.ptr("d_out"), a.ptr("ids"), a.ptr("q"), n, chw,
        _stream()), draw + moved, {"d": d, "u": u, "src": src}, ["ids", "q", "dst", "d_out"],
        verify(S.MULTINOMIAL, S.ONE_Q16, True, False))
    for scheme in (S.STRATIFIED, S.SYSTEMATIC):
        _one("dpsx_resample_draw_seg_ex_f32", lambda a: lib.dpsx_resample_draw_seg_ex_f32(
            a.ptr("d"), a.ptr("u"), 1, n, inv, a.ptr("ids"), a.ptr("q"), scheme, S.ONE_Q16, a.ptr("flag"), a.ptr("ess"),
            _stream()), draw + diag, {"d": d, "u": u}, ["ids", "q", "flag", "ess"], verify(scheme, S.ONE_Q16, False, True))
        _one("dpsx_resample_seg_ex_f32", lambda a: lib.dpsx_resample_seg_ex_f32(
            a.ptr("d"), a.ptr("u"), 1, n, inv, a.ptr("src"), a.ptr("dst"), a.ptr("d_out"), a.ptr("ids"), a.ptr("q"), n, chw,
            scheme, S.ONE_Q16, a.ptr("flag"), a.ptr("ess"), _stream()), draw + moved + diag, {"d": d, "u": u, "src": src},
            ["ids", "q", "dst", "d_out", "flag", "ess"], verify(scheme, S.ONE_Q16, True, True))


# ===================================================================== analysis kernels
# M = 2 images of K = 3 particles, the smallest multi-image shapes of the kernels' own GPU suites, against those suites'
# float64 restatements under those suites' bounds (imported, not restated).  A reduction's partial sums are added in another
# order by the scalar form, so sums are held to the reference, not to the aligned placement's bits; bit for bit are what the
# header says are: the ensemble's mean / var ("the same bits in both forms"), everything of the order statistics ("x ... may
# have any 4-byte alignment"; per-element sorts, integer counts), and mse / psnr of a call with ssim against one without.
AM, AK = 2, 3
ASHAPES = {"3x32x32": (3, 32, 32), "1x16x16": (1, 16, 16)}


def _aset(key):
    c, h, w = ASHAPES[key]
    rng = np.random.RandomState(31 + h)
    label = rng.uniform(-1, 1, (AM, c, h, w)).astype(np.float32)
    x = (np.repeat(label, AK, axis=0) + 0.2 * rng.randn(AM * AK, c, h, w)).astype(np.float32)
    return x, label, AM * AK, c * h * w


def _analysis(name, fn, bufs, inputs, outs, verify, need, bitwise=()):
    bufs = list(bufs) + [Buf("ws", (need,), U8, "ws")]
    movers = [b.name for b in bufs if b.role != "ws" and b.dtype in (F32, U8, I32)]
    return run_case(name, bufs, inputs, [Step(name, fn, outs, ws_refused(True))], verify, movers=movers, ws="ws",
                    bitwise=bitwise)


@pytest.mark.parametrize("key", list(ASHAPES))
def test_image_metrics(K, key):
    import metrics_ref
    from test_metrics_gpu import _close_or_same
    lib, L = _lib()
    x, label, n, d = _aset(key)
    c, h, w = ASHAPES[key]
    names = ["mse", "psnr", "ssim"]
    ref = metrics_ref.metrics(x, label)
    need = int(lib.dpsx_metrics_workspace_bytes(n, AM, c, h, w))
    seen = {}

    def verify(out, ptag):
        _close_or_same(out["mse"], ref["mse"], 1e-5, rel=True)
        _close_or_same(out["psnr"], ref["psnr"], 1e-4)
        if "ssim" in out:
            assert np.abs(out["ssim"] - ref["ssim"]).max() <= 1e-5, ptag
            seen[ptag] = out
        else:           # the squared-error partials of a call without ssim are the same launch geometry and code
            assert np.array_equal(out["mse"], seen[ptag]["mse"]) and np.array_equal(out["psnr"], seen[ptag]["psnr"]), ptag

    _analysis("dpsx_image_metrics_f32", lambda a, wb: lib.dpsx_image_metrics_f32(
        a.ptr("x"), a.ptr("label"), AM, 0.0, a.ptr("mse"), a.ptr("psnr"), a.ptr("ssim"), n, c, h, w, a.ptr("ws"), wb,
        _stream()), [Buf("x", x.shape, F32, "in"), Buf("label", label.shape, F32, "in")] +
        [Buf(k, (n,), F32, "out") for k in names], {"x": x, "label": label}, names, verify, need)
    _analysis("dpsx_image_metrics_f32 (mse, psnr)", lambda a, wb: lib.dpsx_image_metrics_f32(
        a.ptr("x"), a.ptr("label"), AM, 0.0, a.ptr("mse"), a.ptr("psnr"), None, n, c, h, w, a.ptr("ws"), wb, _stream()),
        [Buf("x", x.shape, F32, "in"), Buf("label", label.shape, F32, "in")] + [Buf(k, (n,), F32, "out") for k in names[:2]],
        {"x": x, "label": label}, names[:2], verify, need)


@pytest.mark.parametrize("key", list(ASHAPES))
def test_repulsion(K, key):
    import repulse_ref
    from test_repulse_gpu import _rel
    lib, L = _lib()
    x, _, n, d = _aset(key)
    need = int(lib.dpsx_repulse_workspace_bytes(n, d, AM))
    d2_ref = repulse_ref.sqdist(x, AM)
    iu = np.triu_indices(AK, 1)
    pairs = d2_ref[:, iu[0], iu[1]]
    mean, mn = pairs.mean(axis=1), pairs.min(axis=1)

    def verify_d2(out, ptag):
        d2, info = out["d2"], out["info"]
        assert np.isfinite(d2).all() and _rel(d2, d2_ref) <= 1e-5, ptag
        assert np.array_equal(d2.view(np.uint32), d2.transpose(0, 2, 1).copy().view(np.uint32)), ptag
        assert (np.einsum("mii->mi", d2).view(np.uint32) == 0).all(), ptag
        assert _rel(info[:, 3], mn) <= 1e-5 and _rel(info[:, 2], mean) <= 1e-5, ptag
        assert _rel(info[:, 0], mean / np.log(AK + 1.0)) <= 1e-5 and (info[:, 1] == 0).all(), ptag

    _analysis("dpsx_pairwise_sqdist_f32", lambda a, wb: lib.dpsx_pairwise_sqdist_f32(
        a.ptr("x"), a.ptr("d2"), a.ptr("info"), n, d, AM, a.ptr("ws"), wb, _stream()),
        [Buf("x", (n, d), F32, "in"), Buf("d2", (AM, AK, AK), F32, "out"), Buf("info", (AM, 4), F32, "out")], {"x": x},
        ["d2", "info"], verify_d2, need)
    strength = float(np.float32(0.25 * mean[0] / np.log(AK + 1.0)))        # a quarter of h: a push of a few per cent of x
    ref = repulse_ref.repulse(x, strength, images=AM)

    def verify_push(out, ptag):
        assert (out["applied"] == 1).all() and _rel(out["info"][:, :3], ref["info"][:, :3]) <= 1e-5, ptag
        assert _rel(out["d2"], d2_ref) <= 1e-5, ptag
        u = ref["d2"] / ref["info"][:, 0][:, None, None]
        assert (np.abs(out["w"].astype(np.float64) - ref["w"]) <= (2e-5 * u + 2e-7) * ref["w"] + 2.0 ** -150).all(), ptag
        delta = (out["out"].astype(np.float64) - x.reshape(n, d)).reshape(n, -1)
        dref = ref["delta"].reshape(n, -1)
        floor = np.linalg.norm(0.5 * np.spacing(ref["out"].astype(np.float32)).astype(np.float64).reshape(n, -1), axis=1)
        err, nref = np.linalg.norm(delta - dref, axis=1), np.linalg.norm(dref, axis=1)
        assert (err <= 1e-4 * nref + floor).all(), (ptag, err / nref)

    _analysis("dpsx_repulse_f32", lambda a, wb: lib.dpsx_repulse_f32(
        strength, 0.0, a.ptr("x"), a.ptr("out"), a.ptr("d2"), a.ptr("w"), a.ptr("info"), a.ptr("applied"), n, d, AM,
        a.ptr("ws"), wb, _stream()),
        [Buf("x", (n, d), F32, "in"), Buf("out", (n, d), F32, "out"), Buf("d2", (AM, AK, AK), F32, "out"),
         Buf("w", (AM, AK, AK), F32, "out"), Buf("info", (AM, 4), F32, "out"), Buf("applied", (AM,), U8, "out")], {"x": x},
        ["out", "d2", "w", "info", "applied"], verify_push, need)


@pytest.mark.parametrize("key", list(ASHAPES))
def test_ensemble_statistics(K, key):
    import ensemble_ref
    from test_ensemble_gpu import _check
    lib, L = _lib()
    x, label, n, d = _aset(key)
    ref = ensemble_ref.ensemble(x, images=AM, label=label)
    need = int(lib.dpsx_ensemble_workspace_bytes(n, d, AM))
    maps = ["mean", "var", "mean_lo", "var_lo"]

    def verify(out, ptag):
        got = {"mean": out["mean"].reshape(ref["mean"].shape), "var": out["var"].reshape(ref["var"].shape),
               "info": out["info"], "curve": out["curve"][:, :AK], "final_mse": out["curve"][:, AK]}
        _check({k: v.astype(np.float64) for k, v in got.items()}, ref, f"placement {key} [{ptag}]")

    _analysis("dpsx_ensemble_ex_f32", lambda a, wb: lib.dpsx_ensemble_ex_f32(
        a.ptr("x"), a.ptr("label"), None, 0, a.ptr("mean"), a.ptr("var"), a.ptr("mean_lo"), a.ptr("var_lo"), a.ptr("curve"),
        a.ptr("info"), n, d, AM, a.ptr("ws"), wb, _stream()),
        [Buf("x", (n, d), F32, "in"), Buf("label", (AM, d), F32, "in")] + [Buf(k, (AM, d), F32, "out") for k in maps] +
        [Buf("curve", (AM, AK + 1), F32, "out"), Buf("info", (AM, 4), F32, "out")], {"x": x, "label": label},
        maps + ["curve", "info"], verify, need, bitwise=tuple(maps))


@pytest.mark.parametrize("key", list(ASHAPES))
def test_order_statistics(K, key):
    import ctypes
    import quantile_ref
    from test_quantile_gpu import _close
    lib, L = _lib()
    x, label, n, d = _aset(key)
    probs = (0.05, 0.5, 0.95)
    ref = quantile_ref.order_stats(x, images=AM, probs=probs, label=label)
    need = int(lib.dpsx_quantiles_workspace_bytes(n, d, AM))

    def verify(out, ptag):          # test_quantile_gpu._check's gates: quantiles and histogram bit for bit, 1e-5 on crps / width
        assert np.array_equal(out["quant"].view(np.int32), ref["quantiles"].reshape(AM, 3, d).view(np.int32)), ptag
        assert np.array_equal(out["hist"], ref["hist"]) and (out["hist"].sum(axis=1) == d).all(), ptag
        _close(out["info"][:, 0], ref["info"][:, 0], f"placement {key} [{ptag}] crps")
        _close(out["info"][:, 1], ref["info"][:, 1], f"placement {key} [{ptag}] width")
        assert np.array_equal(out["info"][:, 2:], ref["info"][:, 2:]), ptag

    _analysis("dpsx_quantiles_f32", lambda a, wb: lib.dpsx_quantiles_f32(
        a.ptr("x"), a.ptr("label"), (ctypes.c_double * 3)(*probs), 3, a.ptr("quant"), a.ptr("hist"), a.ptr("info"), n, d, AM,
        a.ptr("ws"), wb, _stream()),
        [Buf("x", (n, d), F32, "in"), Buf("label", (AM, d), F32, "in"), Buf("quant", (AM, 3, d), F32, "out"),
         Buf("hist", (AM, AK + 2), I32, "out"), Buf("info", (AM, 4), F32, "out")], {"x": x, "label": label},
        ["quant", "hist", "info"], verify, need, bitwise=("quant", "hist", "info"))


@pytest.mark.parametrize("key", list(ASHAPES))
def test_principal_components(K, key):
    import pca_ref
    from test_pca_gpu import TAU_L, TAU_N, _bound
    lib, L = _lib()
    x, _, n, d = _aset(key)
    q = 2
    ref = pca_ref.pca(x, images=AM, components=q)
    need = int(lib.dpsx_pca_workspace_bytes(n, d, AM))
    flat = x.reshape(AM, AK, -1).astype(np.float64)
    import repulse_ref
    d2_ref = repulse_ref.sqdist(x, AM)
    from test_repulse_gpu import _rel

    def verify(out, ptag):
        ev, dirs, coords, info = (out[k].astype(np.float64) for k in ("evals", "dirs", "coords", "info"))
        tag = f"placement {key} [{ptag}]"
        assert (info[:, 3] == AK).all() and (info[:, 1] >= 0).all(), tag
        assert np.allclose(info[:, 0], ref["info"][:, 0], rtol=1e-5, atol=0), tag
        assert _rel(out["d2"], d2_ref) <= 1e-5, tag
        for b in range(AM):
            l0 = ref["evals"][b, 0]
            _bound(np.abs(ev[b] - ref["evals"][b]).max() / l0, TAU_L, f"{tag}[{b}]", "eigenvalue")
            xc = flat[b] - flat[b].mean(axis=0)
            for j in np.flatnonzero(ev[b] > 0):
                _bound(abs(np.linalg.norm(dirs[b, j]) - 1), TAU_N, f"{tag}[{b}] u{j}", "norm")
                cj = coords[b, :, j]
                _bound(np.abs(cj - xc @ dirs[b, j]).max() / np.sqrt(l0), TAU_L, f"{tag}[{b}] c{j}", "score")
                assert cj[np.argmax(np.abs(cj))] > 0, tag

    _analysis("dpsx_pca_f32", lambda a, wb: lib.dpsx_pca_f32(
        a.ptr("x"), q, a.ptr("dirs"), a.ptr("evals"), a.ptr("coords"), a.ptr("info"), a.ptr("d2"), n, d, AM, a.ptr("ws"), wb,
        _stream()),
        [Buf("x", (n, d), F32, "in"), Buf("dirs", (AM, q, d), F32, "out"), Buf("evals", (AM, q), F32, "out"),
         Buf("coords", (AM, AK, q), F32, "out"), Buf("info", (AM, 4), F32, "out"), Buf("d2", (AM, AK, AK), F32, "out")],
        {"x": x}, ["dirs", "evals", "coords", "info", "d2"], verify, need)


# ===================================================================== the champion exchange: 16-byte buffers only
def test_champion_exchange_refuses_unaligned_buffers(K, oracle):
    """dpsx_pack_champion_f32 / dpsx_select_champion_f32 exist in the float4 form only: DPSX_EUNSUPPORTED for `particles`,
    `out`, `table` or `dst` off the grid, nothing written; the aligned call runs (chw a multiple of 4)"""
    lib, L = _lib()
    p = _particles(K, oracle, "3x16x16")
    src, costs = p.x.reshape(PN, p.chw), np.array([2.0, 0.5, 1.0], dtype=np.float32)
    rec = np.concatenate([src[1], np.array([0.5, 1.0, 0.0, 0.0], dtype=np.float32)])

    def refuses(names):
        return lambda tag, offs: EUNSUPPORTED if set(names) & set(offs) else OK

    run_case("dpsx_pack_champion_f32", [Buf("particles", (PN, p.chw), F32, "in"), Buf("costs", (PN,), F32, "in"),
                                        Buf("out", (p.chw + 4,), F32, "out")], {"particles": src, "costs": costs},
             [Step("dpsx_pack_champion_f32", lambda a, wb: lib.dpsx_pack_champion_f32(
                 a.ptr("particles"), a.ptr("costs"), None, None, a.ptr("out"), PN, p.chw, _stream()), ["out"],
                 refuses(["particles", "out"]))],
             lambda out, ptag: np.testing.assert_array_equal(out["out"], rec, err_msg=ptag), bitwise=("out",))
    table = np.stack([np.concatenate([src[0], np.array([2.0, 0.0, 0.0, 0.0], dtype=np.float32)]), rec])
    run_case("dpsx_select_champion_f32", [Buf("table", (2, p.chw + 4), F32, "in"), Buf("dst", (2, p.chw), F32, "out"),
                                          Buf("rank", (1,), I64, "out"), Buf("local", (1,), I64, "out")], {"table": table},
             [Step("dpsx_select_champion_f32", lambda a, wb: lib.dpsx_select_champion_f32(
                 a.ptr("table"), 2, p.chw, a.ptr("dst"), 2, a.ptr("rank"), a.ptr("local"), _stream()),
                 ["dst", "rank", "local"], refuses(["table", "dst"]))],
             lambda out, ptag: (np.testing.assert_array_equal(out["dst"], np.stack([src[1], src[1]]), err_msg=ptag),
                                np.testing.assert_array_equal([out["rank"][0], out["local"][0]], [1, 1])),
             bitwise=("dst",))
