"""The refusals of the per-env row entry points that need a handle - a null `out`, bounds that are not finite in float32, rows and delays
the host's admission turns down - by the WHOLE text of nm_last_error(), on one fp32 and one fp64 env of two envs each, no step taken.
After every refusal the env reports what it reported before (the defaults), and a valid call of the same kind still goes through. Only
the fill / get / copy utility kernels run."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import make_env

pytestmark = pytest.mark.gpu
N = 2
BP_MASS = 9      # nm_core.h: the base mass in a body row; the total mass follows it
PAY = ((-1.0, -0.1, -0.1, -0.1), (1.0, 0.1, 0.1, 0.1))
GRAV = ((-0.5, -0.5, -0.5, 0.0, 0.0), (0.5, 0.5, 0.5, 0.3, 6.28))
FRIC = ((0.5, 15.0, 0.6), (1.5, 25.0, 1.0))


def report(env):
    """What the env says about its body rows, gravity rows and delays."""
    g = env.gravity()
    return env.base_payload()["rows"].clone(), g["g"], g["gravity_vec"], env.action_latency()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def call(env, fn, *args):
    return getattr(env._L, fn)(env._h, *args, env._stream())


def ok(env, fn, *args):
    assert call(env, fn, *args) == 0, env._L.nm_last_error().decode()


def refused(env, text, fn, *args, then):
    """The call fails with exactly `text`, the env reports what it did before, and `then` - a valid use of the same kind that ends with
    the kind off again - goes through and leaves the env as it was."""
    before = report(env)
    assert call(env, fn, *args) != 0
    assert env._L.nm_last_error().decode() == text
    assert same(before, report(env)), (fn, text)
    then()
    assert same(before, report(env)), (fn, text)


def bounds(n, lo, hi):
    return C.byref((C.c_double * n)(*lo)), C.byref((C.c_double * n)(*hi))


def big(b):
    """The bounds with the first column's upper one beyond float32."""
    return b[0], (1e39,) + b[1][1:]


def ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_refusals_that_need_a_handle_name_their_fault_and_change_nothing(dtype):
    env = make_env(N, dtype=dtype, seed=5)
    dev = env.device
    fresh = report(env)
    dflt_row = fresh[0][0].clone()
    want_g = torch.tensor([0.0, 0.0, -9.81], dtype=dtype, device=dev).expand(N, 3)
    assert torch.equal(fresh[0][1], dflt_row) and torch.equal(fresh[1], want_g) and torch.equal(fresh[2], want_g) and not fresh[3].any()
    out4, out5 = torch.zeros(N, 4, dtype=dtype, device=dev), torch.zeros(N, 5, dtype=dtype, device=dev)

    # ---- valid uses of each kind, each ending with the kind off again
    def draw_payload():
        out4.zero_()
        ok(env, "nm_draw_payload", *bounds(4, *PAY), ptr(out4))
        assert out4.any() and (out4.abs() <= 1.0).all()

    def draw_gravity():
        out5.zero_()
        ok(env, "nm_draw_gravity", *bounds(5, *GRAV), ptr(out5))
        assert out5.any() and (out5.abs() <= 6.28).all()

    def draw_friction():
        ok(env, "nm_draw_env_params", *bounds(3, *FRIC))
        mu = env.env_params()["mu"]
        assert ((mu >= 0.5) & (mu <= 1.5)).all()
        env.set_env_params()

    rows = dflt_row.expand(N, 20).clone()
    rows[1, BP_MASS:BP_MASS + 2] += 0.5      # mass and total mass

    def set_body():
        ok(env, "nm_set_body_params", ptr(rows))
        assert torch.equal(report(env)[0], rows)
        ok(env, "nm_set_body_params", None)

    g = torch.zeros(N, 8, dtype=dtype, device=dev)
    g[:, 2] = g[:, 6] = -9.81
    g[1, 0] = 1.0

    def set_gravity():
        ok(env, "nm_set_gravity", ptr(g))
        now = report(env)
        assert torch.equal(now[1], g[:, 0:3]) and torch.equal(now[2], g[:, 4:7])
        ok(env, "nm_set_gravity", None)

    top = 3 * int(env.cfg.control.decimation)      # the history holds three env steps
    d = torch.tensor([0, top], dtype=torch.int32, device=dev)

    def set_latency():
        ok(env, "nm_set_action_latency", ptr(d))
        assert torch.equal(report(env)[3], d)
        ok(env, "nm_set_action_latency", None)

    def draw_latency():
        ok(env, "nm_draw_action_latency", top, top)
        assert (report(env)[3] == top).all()
        ok(env, "nm_set_action_latency", None)

    # ---- the draws into the caller's buffer: a null `out`
    refused(env, "nm_draw_payload: out is NULL", "nm_draw_payload", *bounds(4, *PAY), None, then=draw_payload)
    refused(env, "nm_draw_gravity: out is NULL", "nm_draw_gravity", *bounds(5, *GRAV), None, then=draw_gravity)

    # ---- bounds beyond float32: refused on the fp32 env (after `out`), fine on the fp64 env
    if dtype == torch.float32:
        refused(env, "nm_draw_payload: out is NULL", "nm_draw_payload", *bounds(4, *big(PAY)), None, then=draw_payload)
        out4.zero_()
        out5.zero_()
        refused(env, "nm_draw_payload: the bounds of dm must be finite in float32", "nm_draw_payload", *bounds(4, *big(PAY)), ptr(out4),
                then=lambda: None)
        refused(env, "nm_draw_gravity: the bounds of offset x must be finite in float32", "nm_draw_gravity", *bounds(5, *big(GRAV)), ptr(out5),
                then=lambda: None)
        assert not out4.any() and not out5.any()      # a refused draw wrote nothing
        draw_payload()
        draw_gravity()
        refused(env, "nm_draw_env_params: the bounds of mu must be finite in float32", "nm_draw_env_params", *bounds(3, *big(FRIC)), then=draw_friction)
    else:
        ok(env, "nm_draw_payload", *bounds(4, *big(PAY)), ptr(out4))
        ok(env, "nm_draw_gravity", *bounds(5, *big(GRAV)), ptr(out5))
        ok(env, "nm_draw_env_params", *bounds(3, *big(FRIC)))
        assert torch.isfinite(out4).all() and torch.isfinite(out5).all() and torch.isfinite(env.env_params()["mu"]).all()
        assert max(out4[:, 0].abs().max(), out5[:, 0].abs().max(), env.env_params()["mu"].max()) > 1e30      # the wide bound was drawn from
        env.set_env_params()      # friction / gains off again
        assert same(fresh, report(env))

    # ---- rows and delays the admission turns down
    bad = rows.clone()
    bad[1, BP_MASS] = 0.0
    refused(env, "nm_set_body_params: row 1: mass <= 0", "nm_set_body_params", ptr(bad), then=set_body)
    bad = g.clone()
    bad[0, 1] = float("nan")
    refused(env, "nm_set_gravity: row 0: a non-finite value", "nm_set_gravity", ptr(bad), then=set_gravity)
    bad = g.clone()
    bad[1, 4:7] = 0.0
    refused(env, "nm_set_gravity: row 1: a zero gravity_vec", "nm_set_gravity", ptr(bad), then=set_gravity)
    bad = torch.tensor([0, top + 1], dtype=torch.int32, device=dev)
    refused(env, f"nm_set_action_latency: env 1: delay {top + 1} outside [0, {top}] substeps", "nm_set_action_latency", ptr(bad), then=set_latency)
    refused(env, f"nm_draw_action_latency: hi {top + 1} above {top} substeps", "nm_draw_action_latency", 0, top + 1, then=draw_latency)
    assert same(fresh, report(env))

    # ---- a refusal over rows that are set leaves those
    ok(env, "nm_set_body_params", ptr(rows))
    bad = rows.clone()
    bad[0, BP_MASS] = -1.0
    refused(env, "nm_set_body_params: row 0: mass <= 0", "nm_set_body_params", ptr(bad), then=lambda: None)
    assert torch.equal(report(env)[0], rows)
    env.close()
