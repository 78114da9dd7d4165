"""MLP forward on the MFMA units (nm_policy_*): the inference half of rsl_rl's ActorCritic (Linear -> activation ... -> Linear; any
hidden activation of rsl_rl's get_activation, ELU by default), torch.nn.Linear weight layout so state_dicts load unchanged.

Each network owns ONE library handle with a packed copy of its parameters. The copy is refreshed by `repack()`: explicitly (after
an optimiser step, `load_state_dict`, or any write through `.data`) or, in `forward`, whenever the parameters' generation changed -
detected by a cheap fingerprint (data pointers + tensor versions) plus `mark_dirty()` for writes the versions do not see. A HIP graph
that captures `forward` replays the kernel only; after changing weights call `repack()` before the next replay."""
import ctypes as C

import torch

from . import _lib


class PackedMLP:
    """Handle of one packed network on one device (no torch module semantics): load(weights, biases) then forward(obs)."""

    def __init__(self, dims, device, activation="elu"):
        self.dims = [int(d) for d in dims]
        self.device = torch.device(device)
        self.activation = activation
        code = _lib.activation_code(activation)
        if self.device.type != "cuda":
            raise _lib.NightmareHipError("the MLP kernels need a HIP device (no CPU path)")
        self._L = _lib.load()
        h = C.c_void_p()
        arr = (C.c_int32 * len(self.dims))(*self.dims)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self._L.nm_policy_create_act(arr, len(self.dims) - 1, code, idx, C.byref(h)))
        self._h = h
        self._out = None

    def load(self, weights, biases):
        k = len(self.dims) - 1
        assert len(weights) == len(biases) == k
        ws = [w.detach().to(device=self.device, dtype=torch.float32).contiguous() for w in weights]
        bs = [b.detach().to(device=self.device, dtype=torch.float32).contiguous() for b in biases]
        for l in range(k):
            assert tuple(ws[l].shape) == (self.dims[l + 1], self.dims[l]) and tuple(bs[l].shape) == (self.dims[l + 1],)
        wp = (C.c_void_p * k)(*[w.data_ptr() for w in ws])
        bp = (C.c_void_p * k)(*[b.data_ptr() for b in bs])
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self._L.nm_policy_load(self._h, wp, bp, stream))
        self._keep = (ws, bs)     # alive until the stream-ordered copy has run

    def forward(self, obs, out=None):
        if obs.dtype != torch.float32 or not obs.is_contiguous():
            obs = obs.contiguous().float()
        n = obs.shape[0]
        if out is None:
            if self._out is None or self._out.shape[0] != n:
                self._out = torch.empty(n, self.dims[-1], device=self.device, dtype=torch.float32)   # stable address: graph capture
            out = self._out
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self._L.nm_policy_forward(self._h, obs.data_ptr(), n, out.data_ptr(), stream))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.nm_policy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_TORCH_ACT = {"elu": torch.nn.functional.elu, "selu": torch.nn.functional.selu, "relu": torch.relu, "crelu": torch.relu,
              "lrelu": torch.nn.functional.leaky_relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


class ActorMLP(torch.nn.Module):
    """activation: the hidden layers' (a name of rsl_rl's get_activation, as ActorCritic takes it). A checkpoint does not record it."""

    def __init__(self, dims=(66, 256, 256, 18), activation="elu"):
        super().__init__()
        _lib.activation_code(activation)
        self.dims = list(dims)
        self.activation = activation
        self.layers = torch.nn.ModuleList(torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1))
        self._packed = None
        self._generation = None
        self._dirty = True

    def torch_forward(self, x):
        for i, l in enumerate(self.layers):
            x = l(x)
            if i < len(self.layers) - 1:
                x = _TORCH_ACT[self.activation](x)
        return x

    def _fingerprint(self):
        return tuple((p.data_ptr(), p._version) for l in self.layers for p in (l.weight, l.bias))

    def mark_dirty(self):
        """Tell the module its parameters changed in a way tensor versions do not record (writes through `.data`, `dist.broadcast`)."""
        self._dirty = True

    def repack(self):
        dev = self.layers[0].weight.device
        if self._packed is None or self._packed.device != dev:
            self._packed = PackedMLP(self.dims, dev, self.activation)
        self._packed.load([l.weight for l in self.layers], [l.bias for l in self.layers])
        self._generation = self._fingerprint()
        self._dirty = False

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._dirty = True

    @torch.no_grad()
    def forward(self, obs):
        if not obs.is_cuda:
            raise _lib.NightmareHipError("ActorMLP.forward needs a HIP tensor (no CPU path); use torch_forward on the host")
        if self._dirty or self._packed is None or self._generation != self._fingerprint() or self._packed.device != obs.device:
            self.repack()
        return self._packed.forward(obs)


def flat_params_from_state_dict(sd, device):
    """The flat parameter vector the wave policy reads (nm_rollout, nm_play: `actor W0 b0 W1 b1 ..., critic W0 b0 ..., std`) from an
    rsl_rl ActorCritic state_dict (`actor.<2i>.weight/bias`, `critic.<2i>.weight/bias`, `std`; what reference play.py:60-72 loads from
    `model_<it>.pt['model_state_dict']`): a checkpoint is played without a FusedUpdate or an optimizer. Returns (flat float32 device
    tensor, actor dims [n_obs, h1, ..., n_actions])."""
    parts, dims = [], None
    for net in ("actor", "critic"):
        idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith(net + ".") and k.endswith(".weight")})
        if not idx:
            raise KeyError(f"state_dict has no {net}.<i>.weight entries")
        if net == "actor":
            dims = [int(sd[f"actor.{idx[0]}.weight"].shape[1])] + [int(sd[f"actor.{i}.weight"].shape[0]) for i in idx]
        for i in idx:
            parts += [sd[f"{net}.{i}.weight"].reshape(-1), sd[f"{net}.{i}.bias"].reshape(-1)]
    parts.append(sd["std"].reshape(-1))
    flat = torch.cat([p.detach().to(dtype=torch.float32, device="cpu") for p in parts]).to(device).contiguous()
    return flat, dims

