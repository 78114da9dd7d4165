"""Generator of tests/golden/allrand.npz: fp64 reference trajectories with ALL FOUR kinds of per-env rows on at once - gravity vectors,
friction / servo gains, base payloads, actuation latency - which is what cfg.domain_rand gives a user (level 4 of the step, every region of
the row block non-default).

No oracle machinery of its own: the four existing generators composed. Gravity, friction / gains and latency are per-env rows of the
oracle (oracle/nm_oracle.h); the payload is a recompiled model, so each of the four payload sets is ONE library
(make_payload_goldens.payload_lib), and a combined set is that library under its rows. The value sets are IMPORTED from those generators,
not retyped. Combined set k takes gravity set k, friction / gain set (k + 1) % 4, payload set (k + 2) % 4 (the arrangement of
tests/test_gpu_gravity.py set_every_other_kind: no two kinds are aligned across sets; gravity set 3, the unobserved one, stays
unobserved) and the delays DELAYS of make_latency_goldens.py over its eight envs.

Populations (8 envs x T = 10 steps each, per set, free-running), keys those of payload.npz plus `hist`, minus dof_pos and dof_vel, which
this script asserts to equal qpos[..., 7:] and qvel[..., 6:] word for word (with them the file would be 1.15 MiB, above the limit for a
committed file; tests/allrand_tools.py load() derives them again):
    drop   random actions while the robot falls from the initial pose and lands
    stand  SMALL RANDOM actions, new every step, after the robot has settled under such actions (as in latency.npz: zero actions would make
           a delay invisible)
    belly  the robot lying on folded legs while its servos hold the pose: of 80 steps the T consecutive ones with the most env-steps above
           16 contacts
Besides the trajectories the file holds `sets` [4,3] (the gravity, friction / gain and payload set of each combined set), `grav_rows` [4,8],
`envp_rows` [4,3], `payloads` [4,4] (dm, r), `body_rows` [4,20] - every kind's rows as the per-env setters take them - and `delays` [8].

Conditions asserted on the reference alone, before the file is written (all printed):
  * every kind's default rows set (and zero delays) equal no rows set at all, on the same library, bit for bit (the library of payload 0,
    as in make_payload_goldens.py: its constants lie within an ulp of the committed header's, and the trajectories within 1e-12 of
    oracle/libnm_oracle.so's, which is asserted too);
  * every set's `belly` keeps >= 4 env-steps above 16 contacts; no `stand` env resets;
  * ABLATION: per set and kind, the variant with that ONE kind put back to its default, run from the combined run's own recorded start
    state (history included) under the recorded actions - the comparison the free-running tests make. Per env of `drop` and of `stand`, a
    non-default value must take qpos more than 1e-5 away from the combined trajectory (fp64 tolerance 1e-8; fp32 p99 bound 1e-4 on obs);
    where the set carries the kind's default (gravity set 0 in combined set 0, friction set 0 in combined set 3, payload set 0 in
    combined set 2, delay 0 in envs 0 and 7) the ablated variant is still run and must give EQUAL trajectories. Measured smallest
    separations over the envs, drop / stand (m or rad):
        gravity   set 1: 1.3e-02 / 1.6e-02   set 2: 9.3e-03 / 9.6e-03   set 3: 2.0e-02 / 1.6e-02
        friction  set 0: 4.9e-02 / 1.7e-02   set 1: 8.3e-02 / 1.9e-02   set 2: 5.2e-02 / 2.1e-02
        payload   set 0: 2.8e-02 / 9.6e-03   set 1: 4.2e-02 / 1.3e-02   set 3: 4.4e-02 / 1.2e-02
        latency   set 0: 5.7e-02 / 1.4e-02   set 1: 1.1e-01 / 4.4e-03   set 2: 9.7e-02 / 1.4e-02   set 3: 8.8e-02 / 1.4e-02
    (combined set numbers; the delayed envs 1..6 of each).
    The first arrangement tried separates everywhere; nothing was re-chosen.
  * the file is under 1 MiB; nothing but the .npz is written into the tree. The archive's members carry a fixed time stamp, so the file
    is byte-stable.

    python tests/golden/make_allrand_goldens.py            (CPU only; 4 library builds and 27 oracle runs, 8 at a time)
"""
import io
import os
import shutil
import sys
import tempfile
import time
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "allrand.npz")
sys.path.insert(0, HERE)
import make_envparam_goldens as me
import make_gravity_goldens as mg
import make_latency_goldens as ml
import make_payload_goldens as mp
from oracle import oracle as orc      # noqa: E402  (make_envparam_goldens puts the repository root on sys.path)

POPS = ("drop", "stand", "belly")
N, T, H = ml.N, ml.T, ml.H
SEED = 5
DELAYS = ml.DELAYS
KINDS = ("gravity", "friction", "payload", "latency")
SETS = np.array([[k, (k + 1) % 4, (k + 2) % 4] for k in range(4)])      # combined set k: gravity, friction / gain, payload set
SEPARATION = 1e-5
KEYS = ("qpos", "qvel", "qw", "dof_pos", "dof_vel", "act", "cmd", "ep_len", "hist", "actions", "cmd_u", "obs", "rew", "done", "ncon")


def run(lib, grav=None, envp=None, delays=None, src=None):
    """One recording on the library `lib` (None: oracle/libnm_oracle.so) under a gravity set, a friction / gain set (rows of the
    generators' SETS) and delays - each None = never set. src: None = the populations from their own beginnings; otherwise a combined
    run - `drop` and `stand` replayed from ITS recorded start states, histories, actions and command uniforms."""
    rng = np.random.default_rng(SEED)
    many = np.load(os.path.join(HERE, "env_manycontacts.npz"))["init_qpos"][:N]
    default = np.tile([0, np.pi / 5, 0], 6)
    res = {}
    for pop in (POPS if src is None else POPS[:2]):
        o = orc.OracleEnv(N, seed=SEED, lib_path=lib)
        if grav is not None:
            row = mg.row_of(grav)
            o.set_gravity(row[0:3], row[4:7])
        if envp is not None:
            o.set_env_params(envp)
        if delays is not None:
            o.set_action_latency(delays)        # a fresh, zero history
        o.reset_idx()
        if src is not None:
            pick = lambda k: src[f"{pop}_{k}"]
            o.set_state(pick("qpos")[0], pick("qvel")[0], pick("qw")[0])
            o.set_buffers(dof_pos=pick("dof_pos")[0], dof_vel=pick("dof_vel")[0], actions=pick("act")[0], commands=pick("cmd")[0], ep_len=pick("ep_len")[0])
            o.set_action_latency(np.zeros(N, np.int32) if delays is None else delays, pick("hist")[0])
            pre, total = 0, T
        elif pop == "drop":
            pre, total, act = 7, T, lambda: rng.uniform(-1, 1, (N, 18)).astype(np.float32)
        elif pop == "stand":
            pre, total, act = 150, T, lambda: rng.uniform(-0.12, 0.12, (N, 18)).astype(np.float32)
        else:
            o.set_state(many, np.zeros((N, 24)), np.zeros((N, 24)))
            o.set_buffers(dof_pos=many[:, 7:])
            pre, total, act = 0, 80, lambda: np.clip((o.get_buffers()["dof_pos"] + default) / 0.2, -5, 5).astype(np.float32)
        for _ in range(pre):
            o.step(act())
        r = {k: [] for k in KEYS}

        def state():
            q, v, w = o.get_state()
            b = o.get_buffers()
            r["qpos"].append(q); r["qvel"].append(v); r["qw"].append(w); r["dof_pos"].append(b["dof_pos"]); r["dof_vel"].append(b["dof_vel"])
            r["act"].append(b["actions"]); r["cmd"].append(b["commands"]); r["ep_len"].append(b["ep_len"]); r["hist"].append(o.action_history()[0])

        state()
        for t in range(total):
            if src is None:
                a, cu = act(), rng.uniform(0, 1, (N, 4)).astype(np.float32).astype(np.float64)
            else:
                a, cu = src[f"{pop}_actions"][t], src[f"{pop}_cmd_u"][t].astype(np.float64)
            obs, rew, done, _ = o.step(a, cmd_u=cu)
            r["actions"].append(a); r["cmd_u"].append(cu.astype(np.float32)); r["obs"].append(obs.copy()); r["rew"].append(o.rew64.copy())
            r["done"].append(done.astype(np.uint8)); r["ncon"].append(np.array([o.data(i).ncon for i in range(N)], np.uint8))
            state()
        big = (np.stack(r["ncon"]) > 16).sum(axis=1)
        t0 = int(np.argmax([big[i:i + T].sum() for i in range(total - T + 1)]))
        for k in KEYS:
            res[f"{pop}_{k}"] = np.stack(r[k][t0:t0 + T + (len(r[k]) > total)])
    return res


def save_stable(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    t_start = time.time()
    tmp = tempfile.mkdtemp(prefix="nm_allrand_")
    tree_before = sorted(os.listdir(HERE))
    try:
        G, F, P = mg.SETS, me.SETS, mp.SETS
        np.testing.assert_array_equal(G[0], [0, 0, 0, 0, 0, 1]); np.testing.assert_array_equal(F[0], [1.0, 20.0, 0.8]); np.testing.assert_array_equal(P[0], 0.0)
        pool = ThreadPoolExecutor(8)
        libs = list(pool.map(lambda pay: mp.payload_lib(tmp, pay[0], pay[1:]), P))      # (library, body row) per payload set
        print(f"{len(libs)} libraries built")
        zeros = np.zeros(N, np.int32)
        committed, plain, zero = pool.map(lambda a: run(*a), [(None,), (libs[0][0],), (libs[0][0], G[0], F[0], zeros)])
        for key in plain:
            np.testing.assert_array_equal(plain[key], zero[key], err_msg=key)
        print("every kind's default rows set equal no rows set, on the library of payload 0, bit for bit")
        # (that library's header is the payload derivation's for dm = 0, make_payload_goldens.py's set 0: eigh returns the base body's
        # principal axes in another order and the constants within an ulp of the committed ones, so against oracle/libnm_oracle.so there
        # is rounding)
        away = max(np.abs(plain[f"{pop}_qpos"] - committed[f"{pop}_qpos"]).max() for pop in POPS)
        print(f"... and lies within {away:.1e} in qpos of oracle/libnm_oracle.so, the committed header's library")
        assert away < 1e-12

        def combined(k, src=None, without=None):
            """Combined set k, the kind `without` at its default."""
            g, f, p = SETS[k]
            return run(libs[0 if without == "payload" else p][0], G[0 if without == "gravity" else g], F[0 if without == "friction" else f],
                       zeros if without == "latency" else DELAYS, src)

        parts = list(pool.map(combined, range(4)))
        g = {"sets": SETS, "grav_rows": np.stack([mg.row_of(G[s[0]]) for s in SETS]), "envp_rows": np.stack([F[s[1]] for s in SETS]),
             "payloads": np.stack([P[s[2]] for s in SETS]), "body_rows": np.stack([libs[s[2]][1] for s in SETS]), "delays": DELAYS}
        for key in parts[0]:
            g[key] = np.stack([p[key] for p in parts])          # [set, step (T or T + 1), env, ...]
        for pop in POPS:
            big = (g[f"{pop}_ncon"] > 16).sum(axis=(1, 2))
            con = (g[f"{pop}_ncon"] > 0).sum(axis=(1, 2))
            print(f"{pop}: env-steps with contacts per set {con.tolist()}, with more than 16 contacts {big.tolist()}, resets {g[f'{pop}_done'].sum(axis=(1, 2)).tolist()}")
            np.testing.assert_array_equal(g[f"{pop}_hist"][:, 1:, :, 0], g[f"{pop}_act"][:, 1:].astype(np.float32))      # the histories are the scaled, clipped actions
        assert ((g["belly_ncon"] > 16).sum(axis=(1, 2)) >= 4).all(), "every set must exercise the matrix-free layout on several env-steps"
        assert g["stand_done"].sum() == 0, "no standing env of any set may reset in its recorded steps"

        # ---- ablation: one kind back at its default, from the combined run's own start state
        jobs = [(k, kind) for k in range(4) for kind in KINDS]

        replays = list(pool.map(lambda k: combined(k, parts[k]), range(4)))
        for k in range(4):      # the replay from a recorded start state is the recording itself: what was recorded is the whole state
            for pop in POPS[:2]:
                for key in KEYS:
                    np.testing.assert_array_equal(replays[k][f"{pop}_{key}"], g[f"{pop}_{key}"][k], err_msg=f"replay of set {k} {pop} {key}")
        for (k, kind), abl in zip(jobs, pool.map(lambda job: combined(job[0], parts[job[0]], job[1]), jobs)):
            for pop in POPS[:2]:
                sep = np.abs(abl[f"{pop}_qpos"] - g[f"{pop}_qpos"][k]).max(axis=(0, 2))      # per env, over the steps and words
                if kind == "latency":
                    dflt = DELAYS == 0
                else:
                    dflt = np.full(N, SETS[k, KINDS.index(kind)] == 0)
                print(f"set {k} without {kind:8s} {pop:5s}: smallest separation of a non-default env {sep[~dflt].min() if (~dflt).any() else float('nan'):.1e}, "
                      f"largest of a default env {sep[dflt].max() if dflt.any() else float('nan'):.1e}")
                assert (sep[~dflt] > SEPARATION).all(), (k, kind, pop, sep)
                assert (sep[dflt] == 0).all(), (k, kind, pop, sep)
                if dflt.all():
                    for key in KEYS:
                        np.testing.assert_array_equal(abl[f"{pop}_{key}"], g[f"{pop}_{key}"][k], err_msg=f"set {k} {kind} {pop} {key}")
        pool.shutdown()
        # the env layer's joint snapshots ARE the joint words of the state at every recorded instant: they are left out of the file, which
        # would otherwise exceed the size limit, and tests/allrand_tools.py load() puts them back
        for pop in POPS:
            np.testing.assert_array_equal(g[f"{pop}_dof_pos"], g[f"{pop}_qpos"][..., 7:])
            np.testing.assert_array_equal(g.pop(f"{pop}_dof_vel"), g[f"{pop}_qvel"][..., 6:])
            del g[f"{pop}_dof_pos"]
        save_stable(OUT, g)
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes in {time.time() - t_start:.0f} s")
        assert os.path.getsize(OUT) < (1 << 20)
        assert sorted(set(os.listdir(HERE)) - {"allrand.npz", "__pycache__"}) == sorted(set(tree_before) - {"allrand.npz", "__pycache__"})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
