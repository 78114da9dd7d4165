"""The walk over the on / off states of the three kinds of per-env rows - F friction / gains, B body rows (base payload), L actuation
latency - that tests/test_rows_emulated.py (CPU, the emulation shim) and tests/test_gpu_rows.py (the library) both take. Test
infrastructure, like parity_tools.py: the sequence, the values a kind gets each time it is switched on, and the bookkeeping of what an env
that took the walk must hold afterwards.

WALK is an Eulerian circuit of the directed 3-cube: from all-off, each of the 24 single-kind transitions (a kind on or off, from each of
the four states of the other two kinds) occurs exactly once, and the walk ends all-off. So every cross-case of the host's state machine
- clearing friction / gains while a payload is set, switching latency on over rows that were set and cleared before, ... - is walked."""
import numpy as np

WALK = "FFBFFBLFFBFBBLBLLBLFLLBL"


def check_walk():
    seen, state = set(), frozenset()
    for k in WALK:
        seen.add((state, k))
        state = state ^ {k}
    assert len(WALK) == 24 and len(seen) == 24 and not state


class Walk:
    """Iterating yields (toggle index, kind, now on?) after updating `values`: kind -> what is set while it is on (absent while off).
    F: [n,3] rows out of envp_sets, B: [n,4] (dm, rx, ry, rz) out of payloads, L: [n] delays within 0..6. The k-th time a kind is
    switched on, env e gets set (e + k) % 4 (`idx`: kind -> those set numbers), or delay (3 e + k + 1) % 7: neighbours in a wave differ, and so do consecutive visits."""

    def __init__(self, n, envp_sets, payloads):
        self.n, self.sets = n, {"F": np.asarray(envp_sets, np.float64), "B": np.asarray(payloads, np.float64)}
        self.values, self.idx, self.visits = {}, {}, dict(F=0, B=0, L=0)

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
        return "".join(k for k in "FBL" if k in self.values)

    def level(self):
        return 3 if "L" in self.values else 2 if "B" in self.values else 1 if "F" in self.values else 0
