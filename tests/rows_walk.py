"""The walk over the on / off states of the four kinds of per-env rows - F friction / gains, B body rows (base payload), L actuation
latency, G gravity vectors - that tests/test_rows_emulated.py (CPU, the emulation shim) and tests/test_gpu_rows.py (the library) both take.
Test infrastructure, like parity_tools.py: the sequence, the values a kind gets each time it is switched on, and the bookkeeping of what an
env that took the walk must hold afterwards.

WALK is an Eulerian circuit of the directed 4-cube: from all-off, each of the 64 single-kind transitions (a kind on or off, from each of
the eight states of the other three kinds) occurs exactly once, and the walk ends all-off. So every cross-case of the host's state machine
- clearing friction / gains while a payload is set, switching gravity off over latency that was set and cleared before, ... - is walked;
the 24 transitions of the earlier walk over F, B, L are the ones made here while G is off. make_walk() is the routine that produced the
committed string; check_walk() asserts that it still does."""
import numpy as np

KINDS = "FBLG"
WALK = "FFBFFBLFFBFFBLGFFBFFBLFFBFBBLBBLGBBLBLLGLGGLGBGGLGFLLGLGGLGBGGLG"


def make_walk():
    """Hierholzer's algorithm from the all-off state, every state's outgoing edges taken in the order F, B, L, G: deterministic."""
    left = {s: list(KINDS) for s in range(16)}      # state: bit i = kind KINDS[i] is on; the edges not yet taken, in order
    stack, circuit = [(0, "")], []
    while stack:
        s, _ = stack[-1]
        if left[s]:
            k = left[s].pop(0)
            stack.append((s ^ (1 << KINDS.index(k)), k))
        else:
            circuit.append(stack.pop()[1])
    return "".join(reversed(circuit))


def check_walk():
    seen, state = set(), frozenset()
    for k in WALK:
        seen.add((state, k))
        state = state ^ {k}
    assert len(WALK) == 64 and len(seen) == 64 and not state
    assert {(s, k) for s, k in seen if "G" not in s and k != "G"} == {(frozenset(s), k) for s in ("", "F", "B", "L", "FB", "FL", "BL", "FBL") for k in "FBL"}
    assert WALK == make_walk()


class Walk:
    """Iterating yields (toggle index, kind, now on?) after updating `values`: kind -> what is set while it is on (absent while off).
    F: [n,3] rows out of envp_sets, B: [n,4] (dm, rx, ry, rz) out of payloads, L: [n] delays within 0..6, G: [n,8] rows out of
    grav_rows. The k-th time a kind is switched on, env e gets set (e + k) % 4 (`idx`: kind -> those set numbers), or delay
    (3 e + k + 1) % 7: neighbours in a wave differ, and so do consecutive visits."""

    def __init__(self, n, envp_sets, payloads, grav_rows):
        self.n, self.sets = n, {"F": np.asarray(envp_sets, np.float64), "B": np.asarray(payloads, np.float64), "G": np.asarray(grav_rows, np.float64)}
        self.values, self.idx, self.visits = {}, {}, dict(F=0, B=0, L=0, G=0)

    def __iter__(self):
        e = np.arange(self.n)
        for i, k in enumerate(WALK):
            if k in self.values:
                del self.values[k]
            else:
                v = self.visits[k]
                self.visits[k] += 1
                self.idx[k] = (e + v) % 4
                self.values[k] = ((3 * e + v + 1) % 7).astype(np.int32) if k == "L" else self.sets[k][self.idx[k]]
            yield i, k, k in self.values
        assert not self.values

    def on(self):
        return "".join(k for k in KINDS if k in self.values)

    def level(self, physics_only=False):
        """The level a launch takes: G on is 4 either way; L on without G is 3, or 2 when physics-only."""
        v = self.values
        return 4 if "G" in v else (2 if physics_only else 3) if "L" in v else 2 if "B" in v else 1 if "F" in v else 0
