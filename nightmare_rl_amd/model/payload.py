"""Per-env base payload: the model constants of an env whose base body carries a point mass.

A payload is a point mass `dm` (kg, may be negative) rigidly attached to `base_link` at `r` (m, base body frame). An env with payload
(dm, r) behaves as if mjmodel.xml had been recompiled with that mass added to the base: nothing stays stale. What changes:

    base body     m' = m + dm ; ipos' = (m ipos + dm r) / m' ; I' = I + m P(ipos - ipos') + dm P(r - ipos'),  P(d) = (d.d) 1 - d d'
                  (body frame, about the new COM; six words xx yy zz xy xz yz = body_inertia6's order in nm_host_model.h)
    total_mass    + dm
    invweight0    body_invweight0[b][0] of the 7 colliding bodies (base, six tibias): the base floats, so the tibias' values move too
    pgs_scale     1 / (meaninertia' nv)

`payload_rows` derives all of it for N envs at once: M(qpos0) changes only in its 6 x 6 base block (by the point mass's spatial inertia)
and only the base's COM Jacobian depends on the payload. `modified_tables` is the per-env path through compile_model's own functions
(a modified table set, mass_matrix_np / body_jac_com_np again): the reference `payload_rows` is tested against and what the fixture
generator writes headers from.

Row layout (kBodyP = 20 words): ipos3, I6, mass, total_mass, invweight0[7] (collision-table order), pgs_scale, pad.
"""
import numpy as np

from . import compile_model as cm

ROW = 20
C_IPOS, C_I6, C_MASS, C_TOTAL, C_INVW, C_PGS = 0, 3, 9, 10, 11, 18

_cache = {}


def _P(d):
    d = np.asarray(d, dtype=np.float64)
    return np.einsum("...k,...k->...", d, d)[..., None, None] * np.eye(3) - d[..., :, None] * d[..., None, :]


def _base(T):
    """Constants of the committed model that every payload shares."""
    key = id(T)
    if key in _cache:
        return _cache[key]
    q0 = np.asarray(T["qpos0"], dtype=np.float64)
    M, xpos, xmat, Sm, dof_body = cm.mass_matrix_np(T, q0)
    R = cm.quat_to_mat(T["body_iquat"][1])
    I = R @ np.diag(T["body_inertia"][1]) @ R.T
    col = [int(b) for b in T["col_body"]]
    Jt = np.stack([cm.body_jac_com_np(T, q0, b)[0][:3] for b in col[1:]])      # the tibias' COM Jacobians: payload-independent
    c = dict(M=M, xpos=xpos[1].copy(), xmat=xmat[1].copy(), Sm6=Sm[:6].copy(), I=I, m=float(T["body_mass"][1]),
             ipos=np.asarray(T["body_ipos"][1], dtype=np.float64), total=float(np.sum(np.asarray(T["body_mass"])[1:])), Jt=Jt, nv=int(T["nv"]))
    _cache.clear()
    _cache[key] = c
    return c


def _check(dm, r):
    dm = np.atleast_1d(np.asarray(dm, dtype=np.float64))
    r = np.asarray(r, dtype=np.float64)
    if r.ndim == 1:
        r = np.broadcast_to(r, (dm.shape[0], 3))
    if dm.ndim != 1 or r.shape != (dm.shape[0], 3):
        raise ValueError(f"payload: dm must be [N] and r [N,3], got {dm.shape} and {r.shape}")
    if not (np.isfinite(dm).all() and np.isfinite(r).all()):
        raise ValueError("payload: dm and r must be finite")
    return dm, np.ascontiguousarray(r)


def base_body(dm, r, T=None):
    """(m', ipos', I') of the base body with the payload: [N], [N,3], [N,3,3] (body frame, about the new COM). Refuses what MuJoCo's
    compiler refuses: m' <= 0, I' not positive definite, principal moments that violate the triangle inequality."""
    T = T if T is not None else cm.load_tables()
    c = _base(T)
    dm, r = _check(dm, r)
    m1 = c["m"] + dm
    if (m1 <= 0).any():
        raise ValueError(f"payload: the base's mass must stay positive (env {int(np.argmax(m1 <= 0))}: {c['m']:.4f} + {dm[np.argmax(m1 <= 0)]:.4f} kg)")
    ipos1 = (c["m"] * c["ipos"] + dm[:, None] * r) / m1[:, None]
    I1 = c["I"] + c["m"] * _P(c["ipos"] - ipos1) + dm[:, None, None] * _P(r - ipos1)
    w = np.linalg.eigvalsh(I1)                       # ascending
    if (w[:, 0] <= 0).any():
        raise ValueError(f"payload: the base's inertia must stay positive definite (env {int(np.argmax(w[:, 0] <= 0))})")
    if (w[:, 0] + w[:, 1] < w[:, 2]).any():
        raise ValueError(f"payload: the base's principal moments violate the triangle inequality A + B >= C (env {int(np.argmax(w[:, 0] + w[:, 1] < w[:, 2]))})")
    return m1, ipos1, I1


def payload_rows(dm, r, T=None):
    """float64 [N, 20] rows (module docstring) for payloads dm [N] (kg) at r [N,3] (m, base body frame)."""
    T = T if T is not None else cm.load_tables()
    c = _base(T)
    dm, r = _check(dm, r)
    m1, ipos1, I1 = base_body(dm, r, T)
    N, nv = dm.shape[0], c["nv"]
    # M(qpos0): the composite inertia of the base gains the point mass's spatial inertia about the world origin ([ang; lin] ordering)
    p = c["xpos"] + r @ c["xmat"].T
    S = np.zeros((N, 3, 3))
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -p[:, 2], p[:, 1], p[:, 2], -p[:, 0], -p[:, 1], p[:, 0]
    dI = np.zeros((N, 6, 6))
    dI[:, :3, :3] = -dm[:, None, None] * (S @ S)
    dI[:, :3, 3:] = dm[:, None, None] * S
    dI[:, 3:, :3] = -dm[:, None, None] * S
    dI[:, 3:, 3:] = dm[:, None, None] * np.eye(3)
    M = np.broadcast_to(c["M"], (N, nv, nv)).copy()
    M[:, :6, :6] += np.einsum("ia,nab,jb->nij", c["Sm6"], dI, c["Sm6"])
    Minv = np.linalg.inv(M)
    mean = np.einsum("nii->n", M) / nv
    # body_invweight0[b][0] = trace(J M^-1 J')[:3,:3] / 3 with J the COM Jacobian: only the base's depends on the payload
    cb = c["xpos"] + ipos1 @ c["xmat"].T
    Jb = np.zeros((N, 3, nv))
    Jb[:, :, :6] = (c["Sm6"][None, :, 3:] + np.cross(c["Sm6"][None, :, :3], cb[:, None, :])).transpose(0, 2, 1)
    rows = np.zeros((N, ROW))
    rows[:, C_IPOS:C_IPOS + 3] = ipos1
    rows[:, C_I6:C_I6 + 6] = np.stack([I1[:, 0, 0], I1[:, 1, 1], I1[:, 2, 2], I1[:, 0, 1], I1[:, 0, 2], I1[:, 1, 2]], axis=1)
    rows[:, C_MASS] = m1
    rows[:, C_TOTAL] = c["total"] + dm
    rows[:, C_INVW] = np.einsum("nai,nij,naj->n", Jb, Minv, Jb) / 3
    rows[:, C_INVW + 1:C_INVW + 7] = np.einsum("gai,nij,gaj->ng", c["Jt"], Minv, c["Jt"]) / 3
    rows[:, C_PGS] = 1.0 / (mean * nv)
    return rows


def modified_tables(dm, r, T=None):
    """The committed tables with ONE payload compiled in, every constant recomputed through compile_model's own functions: body_mass /
    body_ipos / body_iquat / body_inertia of body 1 (eigh of I', moments descending, a right-handed axis set), body_invweight0 and
    meaninertia. About 25 ms: the per-env reference path."""
    T = dict(T if T is not None else cm.load_tables())
    m1, ipos1, I1 = base_body([float(dm)], np.asarray(r, dtype=np.float64).reshape(1, 3), T)
    w, U = np.linalg.eigh(I1[0])
    order = np.argsort(-w)
    w, U = w[order], U[:, order]
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    for k in ("body_mass", "body_ipos", "body_iquat", "body_inertia"):
        T[k] = np.array(T[k], dtype=np.float64, copy=True)
    T["body_mass"][1], T["body_ipos"][1], T["body_iquat"][1], T["body_inertia"][1] = m1[0], ipos1[0], cm.mat_to_quat(U), w
    q0 = np.asarray(T["qpos0"], dtype=np.float64)
    M = cm.mass_matrix_np(T, q0)[0]
    Minv = np.linalg.inv(M)
    invw = np.zeros((T["nbody"], 2))
    for b in range(1, T["nbody"]):
        J = cm.body_jac_com_np(T, q0, b)[0]
        A = J @ Minv @ J.T
        invw[b] = np.trace(A[:3, :3]) / 3, np.trace(A[3:, 3:]) / 3
    T["meaninertia"] = float(np.mean(np.diag(M)))
    T["body_invweight0"] = invw
    return T


def row_of_tables(T):
    """The [20] row that a table set stands for (the per-env path's answer)."""
    R = cm.quat_to_mat(T["body_iquat"][1])
    I = R @ np.diag(T["body_inertia"][1]) @ R.T
    row = np.zeros(ROW)
    row[C_IPOS:C_IPOS + 3] = T["body_ipos"][1]
    row[C_I6:C_I6 + 6] = I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]
    row[C_MASS] = T["body_mass"][1]
    row[C_TOTAL] = np.sum(np.asarray(T["body_mass"])[1:])
    row[C_INVW:C_INVW + 7] = np.asarray(T["body_invweight0"])[np.asarray(T["col_body"], dtype=int), 0]
    row[C_PGS] = 1.0 / (T["meaninertia"] * T["nv"])
    return row
