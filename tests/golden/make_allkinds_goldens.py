"""Generator of tests/golden/allkinds.npz: fp64 reference trajectories with ALL SEVEN kinds of per-env rows on at once - gravity vectors,
friction / servo gains, base payloads, actuation latency, the servo target model (slew-rate limit, d_gain), the servo torque limit and the
external wrench on the base - which is what cfg.domain_rand plus cfg.control gives a user (level 7 of the step, every region of the row
block non-default).

No oracle machinery of its own: the seven existing generators composed, three levels above make_allrand_goldens.py. Six kinds are
per-env rows of the oracle (oracle/nm_oracle.h); the payload is a recompiled model, so each of the four payload sets is ONE library
(make_payload_goldens.payload_lib), and a combined set is that library under its rows. Value sets are IMPORTED from those generators, not
retyped. Combined set k takes
    gravity set k, friction / gain set (k + 1) % 4, payload set (k + 2) % 4      (make_allrand_goldens.SETS)
    torque set (3, 0, 2, 4)[k] of make_torque_goldens.SETS                       (its KV is not used: kv is the friction set's)
    wrench set (1, 2, 4, 3)[k] of make_wrench_goldens.SETS                       (never the zero wrench)
so each of the four pooled kinds has its default in exactly one set and no set two defaults; env e of the 8 has the delay
make_latency_goldens.DELAYS[e] and the servo row make_servo_goldens.ROWS[e].

Populations are allrand's (same seed, pre-rolls and action streams; 8 envs x T = 10 steps each, per set, free-running): drop, stand,
belly. Kinds 5..7 - the servo model, the torque limit and the wrench - are switched on TOGETHER where the recorded window starts, the
servo model with L = the target of the last late action (make_servo_goldens.py's rule); every pre-roll runs under kinds 1..4 alone, so
every window starts from allrand's own start state. `belly`'s window is chosen from 80 steps as in allrand, the T consecutive steps with
the most env-steps above 16 contacts, counted in what is RECORDED: every start from 0 to 70 is run with the kinds coming on there, and the
first of the best is kept (with kinds 5..7 at their defaults every start gives the same steps, and the rule is allrand's).
What was tried first: limit and wrench acting from a population's first step, as in their own generators. `belly` then keeps 2, 5, 0, 1
env-steps above 16 contacts in the four sets (condition f asks for 4 each), and over all 4 x 4 x 4 assignments of a torque and a wrench
set to a combined set, none had both f and a standing set that saturates (condition c): only the femur limit of 0.3 N m saturates a
standing robot, and a robot lying under it from the start folds away from its many contacts.
With the kinds coming on at the window, the arrangement torque set (k + 3) % 4, wrench set k + 1 meets a..f, but set 2 (limit 3.2 N m on
every joint, kv 1.1) lands with rewards down to -85, and the step writes obs and reward as float32 words: half an ulp there is 3.8e-6,
above the project's fp64 tolerance of 1e-6 for them whatever the kernel computes. Hence condition g, from the number format alone, and
the re-chosen arrangement above: over all 4 x 5 x 4 assignments of a torque and a wrench set to a combined set, the one that keeps f, g
and a saturating standing set, keeps every pooled kind's default in exactly one set, and changes least (sets 2 and 3 take torque sets 2
and 4 for 1 and 2 and swap their wrenches).

Keys: allrand's, plus `lim` per population (the limited targets at every step start, [set, T + 1, 8, 18]), `servo_rows` [8,2],
`torque_rows` [4,3], `wrench_rows` [4,6] (F, tau) and `sensitive` [8 ablations, 4 sets, 2 populations (drop, stand), 8 envs]. Left out
because this script asserts them derivable (tests/allkinds_tools.py load() puts them back): dof_pos, dof_vel (the joint words of qpos,
qvel) and act (row 0 of the step-start history, widened). The end-of-step qfrc_actuator is used for the conditions and left out.

Conditions asserted on the reference alone, before the file is written (all printed; the figures are those of the committed file):
  a  every kind's default rows set equal no rows set at all, on the same library (payload 0's), bit for bit;
  b  with kinds 5..7 at their defaults (servo rows (inf, 0), limits inf, zero wrench) the four combined sets reproduce
     tests/golden/allrand.npz bit for bit in every key the two files share (39 trajectory keys and the six row keys);
  c  ABLATION, eight kinds (the servo row split into rate and d_gain): per set and kind, the variant with that ONE kind at its default,
     replayed from the combined run's own recorded start state (history and lim included) under the recorded actions. sep = max |dqpos|
     per env; `sensitive` = sep > 1e-5, and an insensitive env has sep == 0 (asserted: nothing lies between). Every env carrying the
     kind's default gives EQUAL trajectories. In drop every non-default env is sensitive for every kind; in stand for gravity, friction,
     payload, latency, d_gain and wrench; in stand torque and rate may be insensitive only where the reference has no joint-step that ends
     saturated / no rate-limited joint-step in that env's window, and at least one set each is sensitive. Smallest separation of a
     sensitive env over the sets, drop / stand (m or rad):
         gravity 1.5e-02 / 1.1e-02   friction 4.6e-02 / 1.9e-02   payload 3.4e-02 / 9.2e-03   latency 2.5e-02 / 4.5e-03
         rate    1.0e-01 / 5.4e-04   d_gain   7.6e-03 / 4.3e-04   torque  2.5e-02 / 2.0e-02   wrench  5.5e-03 / 3.4e-03
     stand: torque is sensitive in the 8 envs of set 0 (femur limit 0.3 N m), in 5 envs of set 2 (femur limit 1.6 N m) and in no env of
     set 3, which never saturates standing; rate in envs 1, 2, 4, 6 of every set (envs 3 and 7, rate 0.08: the small actions of `stand` never move a target that far);
  d  the smallest torque saturation margin | |f| - fmax | over finite limits in every recorded window is above 1e-5 N m: 4.1e-04
     (joint-steps that end saturated per set: drop 471, 0, 372, 414; stand 183, 0, 13, 0; belly 210, 0, 108, 44);
  e  the kinds really meet, each count >= 10: joint-steps that end saturated at the torque limit in an env with d_gain > 0 and a non-zero
     delay: 1010; the same in an env whose kv is not the model's: 1357; env-steps with a wrench torque |ipos x Rb' F| > 1e-3 N m in a set
     with a displaced payload COM and a tilted gravity: 240 (sets 1 and 3 have both; set 1's wrench is a pure torque, so all are set 3's);
  f  every set's `belly` keeps >= 4 env-steps above 16 contacts (7, 7, 4, 4); no `stand` env resets;
  g  every recorded obs and reward is below 16 in magnitude, where half an ulp of a float32 word is 4.8e-7, under half the fp64
     tolerance: largest 15.2 (drop), 9.8 (stand), 12.0 (belly).
The file is under 1 MiB (923182 bytes) and byte-stable (make_allrand_goldens.save_stable); nothing but the .npz is written into the tree.

    python tests/golden/make_allkinds_goldens.py            (CPU only; 4 library builds and 46 oracle runs, 8 at a time)
"""
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "allkinds.npz")
sys.path.insert(0, HERE)
import make_allrand_goldens as ma      # noqa: E402  (save_stable, the arrangement of the first four kinds)
import make_envparam_goldens as me      # noqa: E402
import make_gravity_goldens as mg      # noqa: E402
import make_latency_goldens as ml      # noqa: E402
import make_payload_goldens as mp      # noqa: E402
import make_servo_goldens as ms      # noqa: E402
import make_torque_goldens as mt      # noqa: E402
import make_wrench_goldens as mw      # noqa: E402
from oracle import oracle as orc      # noqa: E402  (make_envparam_goldens puts the repository root on sys.path)

POPS = ma.POPS
N, T, H, SEED = ma.N, ma.T, ma.H, ma.SEED
DELAYS, ROWS = ml.DELAYS, ms.ROWS
SETS = ma.SETS                                                       # combined set k: gravity, friction / gain, payload set
TORQUE_SET, WRENCH_SET = (3, 0, 2, 4), (1, 2, 4, 3)                  # the set of make_torque_goldens.SETS / make_wrench_goldens.SETS per combined set
TORQUE = np.stack([mt.SETS[t] for t in TORQUE_SET])                  # [4,3]
WRENCH = np.stack([mw.SETS[w] for w in WRENCH_SET])                  # [4,6]
OUTPUT_BOUND = 16.0      # the step writes obs and reward as float32 words: below 16 half an ulp is 4.8e-7, under half the fp64 tolerance of 1e-6
ABLATIONS = ("gravity", "friction", "payload", "latency", "rate", "d_gain", "torque", "wrench")
SEPARATION = 1e-5
INF = float("inf")
KEYS = ma.KEYS + ("lim", "qfrc", "margin")


def run(lib, grav=None, envp=None, sp=None, src=None):
    """One recording on the library `lib` under a gravity set and a friction / gain set (rows of the generators' SETS; None = never
    set) and sp = dict(delays [8], servo [8,2], fmax [3], wrench [6]), None = none of them ever set ("plain"). src: None = the
    populations from their own beginnings; otherwise a combined run - `drop` and `stand` replayed from ITS recorded start states,
    histories, limited targets, actions and command uniforms."""
    plain = sp is None
    rng = np.random.default_rng(SEED)
    many = np.load(os.path.join(HERE, "env_manycontacts.npz"))["init_qpos"][:N]
    default = np.tile([0, np.pi / 5, 0], 6)
    res = {}

    def begin():
        o = orc.OracleEnv(N, seed=SEED, lib_path=lib)
        if grav is not None:
            row = mg.row_of(grav)
            o.set_gravity(row[0:3], row[4:7])
        if envp is not None:
            o.set_env_params(envp)
        if not plain:
            o.set_action_latency(sp["delays"])        # a fresh, zero history; kinds 5..7 stay at their defaults
        o.reset_idx()
        return o

    def servo_on(o, l0, hist=None):
        """Where the recorded window starts: kinds 5..7 come on together."""
        if not plain:
            if hist is not None:
                o.set_action_latency(sp["delays"], hist)
            o.set_servo(sp["servo"], l0)
            o.set_torque_limit(sp["fmax"])
            o.set_base_wrench(sp["wrench"])

    def record(o, total, actions):
        """`total` recorded steps; actions(t) gives the step's (action, command uniforms)."""
        r = {k: [] for k in KEYS}

        def state():
            q, v, w = o.get_state()
            b = o.get_buffers()
            r["qpos"].append(q); r["qvel"].append(v); r["qw"].append(w); r["dof_pos"].append(b["dof_pos"]); r["dof_vel"].append(b["dof_vel"])
            r["act"].append(b["actions"]); r["cmd"].append(b["commands"]); r["ep_len"].append(b["ep_len"]); r["hist"].append(o.action_history()[0])
            r["lim"].append(o.servo_state()[1])

        state()
        o.torque_limit()      # the margins start here
        for t in range(total):
            a, cu = actions(t)
            obs, rew, done, _ = o.step(a, cmd_u=cu)
            r["actions"].append(a); r["cmd_u"].append(cu.astype(np.float32)); r["obs"].append(obs.copy()); r["rew"].append(o.rew64.copy())
            r["done"].append(done.astype(np.uint8)); r["ncon"].append(np.array([o.data(i).ncon for i in range(N)], np.uint8))
            r["qfrc"].append(np.stack([o.data(i).np("qfrc_actuator")[6:].copy() for i in range(N)]))
            r["margin"].append(np.float64(o.torque_limit()[1].min()))
            state()
        return r

    draw_cu = lambda: rng.uniform(0, 1, (N, 4)).astype(np.float32).astype(np.float64)
    for pop in (POPS if src is None else POPS[:2]):
        o = begin()
        if src is not None:
            pick = lambda k: src[f"{pop}_{k}"]
            o.set_state(pick("qpos")[0], pick("qvel")[0], pick("qw")[0])
            o.set_buffers(dof_pos=pick("dof_pos")[0], dof_vel=pick("dof_vel")[0], actions=pick("act")[0], commands=pick("cmd")[0], ep_len=pick("ep_len")[0])
            servo_on(o, pick("lim")[0], pick("hist")[0])
            r = record(o, T, lambda t: (src[f"{pop}_actions"][t], src[f"{pop}_cmd_u"][t].astype(np.float64)))
        elif pop != "belly":
            pre, amp = (7, 1.0) if pop == "drop" else (150, 0.12)
            act = lambda: rng.uniform(-amp, amp, (N, 18)).astype(np.float32)
            past = []      # the scaled and clipped actions of the pre-roll, the oracle's own buffer after each step
            for _ in range(pre):
                o.step(act())
                past.append(o.get_buffers()["actions"].copy())
            if not plain:      # the servo model comes on here, holding the target of the last late action a_{t-1-k}
                k = sp["delays"] // ms.DECIMATION
                servo_on(o, np.stack([past[-1 - k[e]][e] - ms.DEFAULT_POS for e in range(N)]))
            r = record(o, T, lambda t: (act(), draw_cu()))
        else:
            hold = lambda t: (np.clip((o.get_buffers()["dof_pos"] + default) / 0.2, -5, 5).astype(np.float32), draw_cu())
            rng_state = rng.bit_generator.state
            best = -1
            for t0 in range(1 if plain else 80 - T + 1):      # every place the window can start: the model comes on there
                if t0 > 0:
                    o = begin()
                rng.bit_generator.state = rng_state
                o.set_state(many, np.zeros((N, 24)), np.zeros((N, 24)))
                o.set_buffers(dof_pos=many[:, 7:])
                past = [np.zeros((N, 18))] * (H + 1)      # before the first step the history is zero
                for t in range(t0):
                    a, cu = hold(t)
                    o.step(a, cmd_u=cu)
                    past.append(o.get_buffers()["actions"].copy())
                if not plain:
                    k = sp["delays"] // ms.DECIMATION
                    servo_on(o, np.stack([past[-1 - k[e]][e] - ms.DEFAULT_POS for e in range(N)]))
                cand = record(o, 80 if plain else T, hold)
                big = (np.stack(cand["ncon"]) > 16).sum(axis=1)
                if plain:      # no servo model to switch on: allrand's single pass
                    w0 = int(np.argmax([big[i:i + T].sum() for i in range(80 - T + 1)]))
                    cand = {k_: v[w0:w0 + T + (len(v) > 80)] for k_, v in cand.items()}
                elif big.sum() <= best:
                    continue
                r, best = cand, int(big.sum())
        for k_ in KEYS:
            res[f"{pop}_{k_}"] = np.stack(r[k_])
    return res


def main():
    t_start = time.time()
    tmp = tempfile.mkdtemp(prefix="nm_allkinds_")
    tree_before = sorted(os.listdir(HERE))
    try:
        G, F, P = mg.SETS, me.SETS, mp.SETS
        np.testing.assert_array_equal(G[0], [0, 0, 0, 0, 0, 1]); np.testing.assert_array_equal(F[0], [1.0, 20.0, 0.8]); np.testing.assert_array_equal(P[0], 0.0)
        assert np.isinf(mt.SETS[0]).all() and not mw.SETS[0].any() and (ROWS[0] == [INF, 0.0]).all() and DELAYS[0] == 0
        defaults = [int(SETS[k, 0] == 0) + int(SETS[k, 1] == 0) + int(SETS[k, 2] == 0) + int(np.isinf(TORQUE[k]).all()) for k in range(4)]
        assert defaults == [1, 1, 1, 1] and WRENCH.any(axis=1).all(), "each pooled kind has its default in exactly one set, no set two"
        pool = ThreadPoolExecutor(8)
        libs = list(pool.map(lambda pay: mp.payload_lib(tmp, pay[0], pay[1:]), P))      # (library, body row) per payload set
        print(f"{len(libs)} libraries built")
        nruns = [0]
        DEFAULTS = dict(delays=np.zeros(N, np.int32), servo=ms.DEFAULT_ROWS, fmax=mt.SETS[0], wrench=mw.SETS[0])

        def combined(k, src=None, without=None, **over):
            """Combined set k under its rows, the kind `without` (one of ABLATIONS) at its default, single kinds overridden."""
            g, f, p = SETS[k]
            sp = dict(delays=DELAYS, servo=ROWS, fmax=TORQUE[k], wrench=WRENCH[k])
            sp.update({"latency": dict(delays=DEFAULTS["delays"]), "rate": dict(servo=no_rate), "d_gain": dict(servo=no_dgain),
                       "torque": dict(fmax=DEFAULTS["fmax"]), "wrench": dict(wrench=DEFAULTS["wrench"])}.get(without, {}))
            sp.update(over)
            nruns[0] += 1
            return run(libs[0 if without == "payload" else p][0], G[0 if without == "gravity" else g], F[0 if without == "friction" else f], sp, src)

        no_rate, no_dgain = ROWS.copy(), ROWS.copy()
        no_rate[:, 0], no_dgain[:, 1] = INF, 0.0
        # ---- a
        plain, zero = pool.map(lambda a: run(libs[0][0], *a), [(), (G[0], F[0], DEFAULTS)])
        nruns[0] += 2
        for key in plain:
            np.testing.assert_array_equal(plain[key], zero[key], err_msg=key)
        print("a: every kind's default rows set equal no rows set, on the library of payload 0, bit for bit")
        # ---- b
        allrand = np.load(os.path.join(HERE, "allrand.npz"))
        lower = list(pool.map(lambda k: combined(k, servo=DEFAULTS["servo"], fmax=DEFAULTS["fmax"], wrench=DEFAULTS["wrench"]), range(4)))
        shared = 0
        for key in allrand.files:
            if key.split("_")[0] in POPS:
                np.testing.assert_array_equal(np.stack([p[key] for p in lower]), allrand[key], err_msg=key)
                shared += 1
        print(f"b: with kinds 5..7 at their defaults the four combined sets equal allrand.npz bit for bit in its {shared} trajectory keys")

        # ---- the combined runs
        parts = list(pool.map(combined, range(4)))
        g = {"sets": SETS, "grav_rows": np.stack([mg.row_of(G[s[0]]) for s in SETS]), "envp_rows": np.stack([F[s[1]] for s in SETS]),
             "payloads": np.stack([P[s[2]] for s in SETS]), "body_rows": np.stack([libs[s[2]][1] for s in SETS]), "delays": DELAYS,
             "servo_rows": ROWS, "torque_rows": TORQUE, "wrench_rows": WRENCH}
        for key in ("sets", "grav_rows", "envp_rows", "payloads", "body_rows", "delays"):
            np.testing.assert_array_equal(g[key], allrand[key], err_msg=key)
        for key in parts[0]:
            g[key] = np.stack([p[key] for p in parts])          # [set, step (T or T + 1), env, ...]
        for pop in POPS:
            big = (g[f"{pop}_ncon"] > 16).sum(axis=(1, 2))
            con = (g[f"{pop}_ncon"] > 0).sum(axis=(1, 2))
            print(f"{pop}: env-steps with contacts per set {con.tolist()}, with more than 16 contacts {big.tolist()}, resets {g[f'{pop}_done'].sum(axis=(1, 2)).tolist()}")
        assert ((g["belly_ncon"] > 16).sum(axis=(1, 2)) >= 4).all(), "f: every set must exercise the matrix-free layout on several env-steps"
        assert g["stand_done"].sum() == 0, "f: no standing env of any set may reset in its recorded steps"
        print("f: holds")
        top = {pop: max(float(np.abs(g[f"{pop}_{key}"]).max()) for key in ("obs", "rew")) for pop in POPS}
        print("g: largest |obs| or |reward| " + ", ".join(f"{pop} {v:.1f}" for pop, v in top.items()))
        assert max(top.values()) < OUTPUT_BOUND, "g"

        # ---- d, e
        limit18 = np.tile(TORQUE, (1, 6))[:, None, None, :]                                    # [set, 1, 1, 18]
        sat = {pop: np.abs(g[f"{pop}_qfrc"]) >= limit18 for pop in POPS}                         # [set, T, env, 18] ends saturated
        margin = min(g[f"{pop}_margin"].min() for pop in POPS)
        print(f"d: smallest torque saturation margin over every recorded window {margin:.2e} N m; saturated joint-steps per set "
              + ", ".join(f"{pop} {sat[pop].sum(axis=(1, 2, 3)).tolist()}" for pop in POPS))
        assert margin > 1e-5, "d"
        both = (ROWS[:, 1] > 0) & (DELAYS > 0)
        own_kv = g["envp_rows"][:, 2] != F[0, 2]
        n1 = sum(int(sat[pop][:, :, both].sum()) for pop in POPS)
        n2 = sum(int(sat[pop][own_kv].sum()) for pop in POPS)
        meet = (g["payloads"][:, 1:] != 0).any(axis=1) & (g["grav_rows"][:, 0:2] != 0).any(axis=1)
        n3 = 0
        for pop in POPS:
            q = g[f"{pop}_qpos"][:, :T, :, 3:7]                                                 # the base's quaternion at each step start
            w, x, y, z = (q[..., i] for i in range(4))
            R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                          np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                          np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)      # [set, T, env, 3, 3]
            Fb = np.einsum("steji,sj->stei", R, WRENCH[:, 0:3])                                  # Rb' F
            tq = np.cross(np.broadcast_to(g["body_rows"][:, None, None, 0:3], Fb.shape), Fb)
            n3 += int((np.abs(tq).max(axis=-1) > 1e-3)[meet].sum())
        print(f"e: joint-steps ending saturated in an env with d_gain > 0 and a delay {n1}, in an env whose kv is not the model's {n2}; "
              f"env-steps with |ipos x Rb' F| > 1e-3 N m in a set with a displaced payload COM and a tilted gravity {n3} (sets {np.flatnonzero(meet).tolist()})")
        assert min(n1, n2, n3) >= 10, "e"

        # ---- c: one kind back at its default, from the combined run's own start state
        replays = list(pool.map(lambda k: combined(k, parts[k]), range(4)))
        for k in range(4):      # the replay from a recorded start state is the recording itself: what was recorded is the whole state
            for pop in POPS[:2]:
                for key in KEYS:
                    np.testing.assert_array_equal(replays[k][f"{pop}_{key}"], g[f"{pop}_{key}"][k], err_msg=f"replay of set {k} {pop} {key}")
        jobs = [(k, kind) for k in range(4) for kind in ABLATIONS]
        sensitive = np.zeros((len(ABLATIONS), 4, 2, N), np.uint8)
        smallest = np.full((len(ABLATIONS), 2), INF)
        for (k, kind), abl in zip(jobs, pool.map(lambda job: combined(job[0], parts[job[0]], job[1]), jobs)):
            a = ABLATIONS.index(kind)
            dflt = {"latency": DELAYS == 0, "rate": np.isinf(ROWS[:, 0]), "d_gain": ROWS[:, 1] == 0, "torque": np.full(N, np.isinf(TORQUE[k]).all()),
                    "wrench": np.full(N, not WRENCH[k].any())}.get(kind)
            if dflt is None:
                dflt = np.full(N, SETS[k, a] == 0)
            for p, pop in enumerate(POPS[:2]):
                sep = np.abs(abl[f"{pop}_qpos"] - g[f"{pop}_qpos"][k]).max(axis=(0, 2))      # per env, over the steps and words
                sens = sep > SEPARATION
                sensitive[a, k, p] = sens
                print(f"c: set {k} without {kind:8s} {pop:5s}: smallest separation of a non-default env {sep[~dflt].min() if (~dflt).any() else float('nan'):.1e}, "
                      f"largest of a default env {sep[dflt].max() if dflt.any() else float('nan'):.1e}, sensitive {sens.astype(int).tolist()}")
                assert (sep[dflt] == 0).all(), (k, kind, pop, sep)
                assert ((sep == 0) | sens).all(), (k, kind, pop, sep)      # insensitive is EQUAL: no env lies between the tolerances
                if sens.any():
                    smallest[a, p] = min(smallest[a, p], sep[sens].min())
                if pop == "drop" or kind not in ("torque", "rate"):
                    assert sens[~dflt].all(), (k, kind, pop, sep)
                elif kind == "torque":      # insensitive only where no joint-step of the env's window ends saturated
                    assert not (~sens & sat[pop][k].any(axis=(0, 2)))[~dflt].any(), (k, kind, pop, sep)
                else:      # insensitive only where the limiter never cut a target short in the env's window
                    cut = ms.saturation({key: v[k] for key, v in g.items() if key.startswith(pop)}, pop, DELAYS).any(axis=(0, 2))
                    assert not (~sens & cut)[~dflt].any(), (k, kind, pop, sep, cut)
                if dflt.all():
                    for key in KEYS:
                        np.testing.assert_array_equal(abl[f"{pop}_{key}"], g[f"{pop}_{key}"][k], err_msg=f"set {k} {kind} {pop} {key}")
        for kind in ("torque", "rate"):
            s = sensitive[ABLATIONS.index(kind), :, 1]
            print(f"c: stand, {kind}: sensitive envs per set {s.sum(axis=1).tolist()}")
            assert s.any(), (kind, "at least one set must be sensitive in stand")
        print("c: smallest separation of a sensitive env, drop / stand: " + "   ".join(f"{kind} {smallest[a, 0]:.1e} / {smallest[a, 1]:.1e}" for a, kind in enumerate(ABLATIONS)))
        pool.shutdown()
        g["sensitive"] = sensitive
        # what is left out: the conditions' inputs, and what tests/allkinds_tools.py load() derives again
        for pop in POPS:
            del g[f"{pop}_qfrc"], g[f"{pop}_margin"]
            np.testing.assert_array_equal(g.pop(f"{pop}_dof_pos"), g[f"{pop}_qpos"][..., 7:])
            np.testing.assert_array_equal(g.pop(f"{pop}_dof_vel"), g[f"{pop}_qvel"][..., 6:])
            np.testing.assert_array_equal(g.pop(f"{pop}_act"), g[f"{pop}_hist"][:, :, :, 0].astype(np.float64))
        ma.save_stable(OUT, g)
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes in {time.time() - t_start:.0f} s, {len(libs)} library builds, {nruns[0]} oracle runs")
        assert os.path.getsize(OUT) < (1 << 20)
        assert sorted(set(os.listdir(HERE)) - {"allkinds.npz", "__pycache__"}) == sorted(set(tree_before) - {"allkinds.npz", "__pycache__"})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
