"""NativePolicy — an MLP actor-critic the device evaluates inside the rollout (ssg_policy_act / ssg_rollout_policy, ABI 9).

The reference's runner does one policy forward + action sampling per ``env.step`` (train/stable_baselines/ppo.py:84-100); a
GPU-resident trainer does the same with a dozen PyTorch kernels per step.  ``NativePolicy`` hands the parameters of such a network
to the library as ONE packed f32 device buffer — ``torch.cat([p.flatten() for p in net.parameters()])`` of an ActorCritic shaped
like train/ppo_torch.py's: ``body = Sequential(Linear, Tanh|ReLU[, Linear, Tanh|ReLU])``, heads ``pi`` (n_actions) and ``v`` (1) —
plus the f64 observation scale.  ``refresh()`` re-packs it in place (same address) after an optimiser step.

The reference trainers' own shape has a value network of its own (Stable-Baselines' ``MlpPolicy``: two 64-64 tanh towers; RLlib's
default ``vf_share_layers=False``): ``pi_body`` and ``vf_body`` of one depth, width and activation, heads ``pi`` on the first and ``v``
on the second, declared in the order ``pi_body, pi, vf_body, v``.  ``value_layers`` / ``from_actor_critic`` take that shape too
(SSG_POLICY_SEPARATE_VALUE in the record's ``activation``).

``ShipVecEnv.policy_act`` / ``ShipVecEnv.rollout_policy`` run it.  ``forward_reference`` is a plain torch restatement for tests.
"""
import ctypes as C

from . import _native as N
from ._native import _torch

ACTIVATIONS = {"tanh": N.POLICY_TANH, "relu": N.POLICY_RELU}


def packed_offsets(obs_dim, hidden, n_hidden_layers, n_actions, separate_value=False):
    """{name: (offset, shape)} of every tensor inside the packed buffer (include/shipsim.h, ssg_policy), and the total length.
    separate_value: the vf tower V0, c0[, V1, c1] sits between the pi head and the v head."""
    D, H, A = int(obs_dim), int(hidden), int(n_actions)
    shapes = [("W0", (H, D)), ("b0", (H,))]
    if n_hidden_layers == 2:
        shapes += [("W1", (H, H)), ("b1", (H,))]
    shapes += [("Wpi", (A, H)), ("bpi", (A,))]
    if separate_value:
        shapes += [("V0", (H, D)), ("c0", (H,))]
        if n_hidden_layers == 2:
            shapes += [("V1", (H, H)), ("c1", (H,))]
    shapes += [("Wv", (1, H)), ("bv", (1,))]
    out, o = {}, 0
    for name, shp in shapes:
        out[name] = (o, shp)
        n = 1
        for s in shp:
            n *= s
        o += n
    return out, o


class NativePolicy(object):
    """layers: [(W0, b0)] or [(W0, b0), (W1, b1)] with W [out][in] (nn.Linear's order); pi, v: (W, b) of the heads; obs_scale: f64
    [obs_dim] (or a number) — the device computes x = (float)(obs / obs_scale) as train/ppo_torch.py's normalise() does.
    value_layers: None = `v` sits on `layers` (the shared body); otherwise the vf tower, a list of (W, b) shaped like `layers`, with
    `pi` on `layers` and `v` on `value_layers`."""

    def __init__(self, layers, pi, v, obs_scale, activation="tanh", value_layers=None):
        torch = _torch()
        if activation not in ACTIVATIONS:
            raise ValueError("activation must be 'tanh' or 'relu' (got %r)" % (activation,))
        layers = [tuple(l) for l in layers]
        if len(layers) not in (1, 2):
            raise ValueError("NativePolicy: 1 or 2 hidden layers (got %d)" % len(layers))
        W0 = layers[0][0]
        if W0.dim() != 2:
            raise ValueError("NativePolicy: weights must be [out][in] matrices")
        H, D = int(W0.shape[0]), int(W0.shape[1])
        if H < 16 or H > N.POLICY_MAX_HIDDEN or H % 16:
            raise ValueError("NativePolicy: hidden width must be a multiple of 16 in 16..%d (got %d)" % (N.POLICY_MAX_HIDDEN, H))
        A = int(pi[0].shape[0])
        if A < 2 or A > 4:
            raise ValueError("NativePolicy: n_actions must be in 2..4 (ssg_step accepts actions 0..3; got %d)" % A)
        tower = [((H, D), (H,))] + [((H, H), (H,))] * (len(layers) - 1)
        self.separate_value = value_layers is not None
        value_layers = [tuple(l) for l in value_layers] if self.separate_value else []
        if self.separate_value and len(value_layers) != len(layers):
            raise ValueError("NativePolicy: value_layers has %d layers, layers %d (both towers must have the same depth)"
                             % (len(value_layers), len(layers)))
        # (a vf tower of another width fails the shape check below)
        ordered = layers + [tuple(pi)] + value_layers + [tuple(v)]  # the packed order
        want = tower + [((A, H), (A,))] + (tower if self.separate_value else []) + [((1, H), (1,))]
        for (W, b), (ws, bs) in zip(ordered, want):
            if tuple(W.shape) != ws or tuple(b.shape) != bs:
                raise ValueError("NativePolicy: a (W, b) pair has shapes %s, %s where %s, %s belong" % (tuple(W.shape), tuple(b.shape), ws, bs))
            if W.dtype != torch.float32 or b.dtype != torch.float32 or W.device != W0.device or b.device != W0.device:
                raise ValueError("NativePolicy: every parameter must be float32 on one device")
        self.obs_dim, self.hidden, self.n_hidden_layers, self.n_actions = D, H, len(layers), A
        self.activation = activation
        self.device = W0.device
        self._sources = [t for pair in ordered for t in pair]
        self.offsets, total = packed_offsets(D, H, len(layers), A, self.separate_value)
        with torch.no_grad():
            self.params = torch.empty(total, dtype=torch.float32, device=self.device)
            self.refresh()
            if not torch.is_tensor(obs_scale):
                obs_scale = torch.full((D,), float(obs_scale), dtype=torch.float64)
            obs_scale = obs_scale.detach().to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        if obs_scale.numel() != D:
            raise ValueError("NativePolicy: obs_scale has %d entries, obs_dim is %d" % (obs_scale.numel(), D))
        self.obs_scale = obs_scale

    @classmethod
    def from_actor_critic(cls, net, obs_scale):
        """A NativePolicy over the parameters OF `net` (refresh() picks up their new values after an optimiser step).  `net` must be
        shaped like train/ppo_torch.py's ActorCritic, in one of its two shapes: ``body, pi, v`` (shared) or ``pi_body, pi, vf_body, v``
        (separate value network); anything else raises ValueError."""
        nn = _torch().nn
        shapes = "expected a module with body = nn.Sequential, pi = nn.Linear, v = nn.Linear (shared body), or with pi_body, vf_body = " \
                 "nn.Sequential of one depth, width and activation, pi = nn.Linear, v = nn.Linear (separate value network)"
        body, pi, v = getattr(net, "body", None), getattr(net, "pi", None), getattr(net, "v", None)
        pi_body, vf_body = getattr(net, "pi_body", None), getattr(net, "vf_body", None)
        separate = pi_body is not None or vf_body is not None
        if separate and body is not None:
            raise ValueError("from_actor_critic: the module has both body and pi_body / vf_body; " + shapes)
        if not isinstance(pi, nn.Linear) or not isinstance(v, nn.Linear):
            raise ValueError("from_actor_critic: " + shapes)
        bodies = [pi_body, vf_body] if separate else [body]
        if not all(isinstance(b, nn.Sequential) for b in bodies):
            raise ValueError("from_actor_critic: " + shapes)
        acts = {nn.Tanh: "tanh", nn.ReLU: "relu"}
        kinds = set()
        towers = []
        for b in bodies:
            mods = list(b)
            if len(mods) not in (2, 4):
                raise ValueError("from_actor_critic: a body must be Linear, act[, Linear, act] (1 or 2 hidden layers; got %d modules)" % len(mods))
            layers = []
            for lin, act in zip(mods[0::2], mods[1::2]):
                if not isinstance(lin, nn.Linear) or type(act) not in acts or lin.bias is None:
                    raise ValueError("from_actor_critic: a body must alternate nn.Linear (with bias) and nn.Tanh / nn.ReLU (got %s, %s)"
                                     % (type(lin).__name__, type(act).__name__))
                kinds.add(acts[type(act)])
                layers.append((lin.weight, lin.bias))
            towers.append(layers)
        if len(kinds) != 1:
            raise ValueError("from_actor_critic: every hidden layer (of both towers) must use the same activation; " + shapes)
        if pi.bias is None or v.bias is None or v.out_features != 1:
            raise ValueError("from_actor_critic: heads must be nn.Linear with bias, v with one output")
        if separate:
            if len(towers[0]) != len(towers[1]) or towers[0][0][0].shape != towers[1][0][0].shape:
                raise ValueError("from_actor_critic: pi_body and vf_body differ in depth or width; " + shapes)
            names = [n for n, _ in net.named_children() if n in ("pi_body", "pi", "vf_body", "v")]
            if names != ["pi_body", "pi", "vf_body", "v"]:
                raise ValueError("from_actor_critic: the module must declare pi_body, pi, vf_body, v in that order (the packed layout is "
                                 "torch.cat of its parameters()); got %s" % names)
        return cls(towers[0], (pi.weight, pi.bias), (v.weight, v.bias), obs_scale, activation=kinds.pop(),
                   value_layers=towers[1] if separate else None)

    def refresh(self):
        """Re-pack the parameters into the same device buffer (one torch.cat): call after every optimiser step."""
        torch = _torch()
        with torch.no_grad():
            torch.cat([t.detach().reshape(-1) for t in self._sources], out=self.params)
        return self.params

    # ------------------------------------------------------------------------------------------------
    # state (ship_sim_gym_amd/checkpoint.py)
    # ------------------------------------------------------------------------------------------------
    def architecture(self):
        """The fields that fix the packed layout, as (name, value) pairs: what a state must agree with."""
        return [("obs_dim", self.obs_dim), ("hidden", self.hidden), ("n_hidden_layers", self.n_hidden_layers),
                ("n_actions", self.n_actions), ("activation", self.activation), ("separate_value", bool(self.separate_value))]

    def state_dict(self):
        """The architecture, the packed parameters and the observation scale (CPU copies; plain data only)."""
        sd = dict(self.architecture())
        sd["params"], sd["obs_scale"] = self.params.detach().cpu().clone(), self.obs_scale.detach().cpu().clone()
        return sd

    def load_state_dict(self, sd):
        """Take a state_dict's parameters and observation scale, in place (``params`` keeps its address).  Everything is checked first:
        an architecture field, a shape or a dtype that differs raises ValueError naming the field with both values, and the object
        stays as it was.  The tensors this policy was built over (a module's parameters, for ``from_actor_critic``) get the loaded
        values as well, so that a later ``refresh()`` re-packs what was loaded."""
        from .checkpoint import check_state
        check_state("NativePolicy.load_state_dict", sd, self.architecture(), [("params", self.params), ("obs_scale", self.obs_scale)])
        with _torch().no_grad():
            self.params.copy_(sd["params"])
            self.obs_scale.copy_(sd["obs_scale"])
            self.push_sources()
        return self

    def push_sources(self):
        """The reverse of ``refresh()``: copy the packed buffer into the tensors it was packed from."""
        o = 0
        with _torch().no_grad():
            for t in self._sources:
                t.copy_(self.params[o: o + t.numel()].view_as(t))
                o += t.numel()

    @classmethod
    def from_state_dict(cls, sd, device, row=None):
        """A NativePolicy on `device` built from a state_dict alone (no module): the architecture comes from the state.  row: for a
        NativePopulation's state, the member whose row of ``params`` to take."""
        torch = _torch()
        from .checkpoint import check_values
        who = "NativePolicy.from_state_dict"
        if not isinstance(sd, dict):
            raise ValueError("%s: a state dict is a dict (got a %s)" % (who, type(sd).__name__))
        check_values(who, sd, [("obs_dim", int), ("hidden", int), ("n_hidden_layers", int), ("n_actions", int), ("activation", str),
                               ("separate_value", bool)])
        params, scale = sd.get("params"), sd.get("obs_scale")
        if not torch.is_tensor(params) or not torch.is_tensor(scale):
            raise ValueError("%s: params and obs_scale must be tensors" % who)
        if row is not None:
            if params.dim() != 2 or not 0 <= int(row) < params.shape[0]:
                raise ValueError("%s: member %r of a params tensor %s" % (who, row, tuple(params.shape)))
            params = params[int(row)]
        D, H, L, A = sd["obs_dim"], sd["hidden"], sd["n_hidden_layers"], sd["n_actions"]
        if L not in (1, 2) or D < 1 or H < 1 or A < 1:
            raise ValueError("%s: obs_dim %d, hidden %d, n_hidden_layers %d, n_actions %d is no architecture" % (who, D, H, L, A))
        offsets, total = packed_offsets(D, H, L, A, sd["separate_value"])
        if params.dtype != torch.float32 or params.dim() != 1 or params.numel() != total:
            raise ValueError("%s: params is a %s tensor %s, the architecture packs into float32 (%d,)"
                             % (who, params.dtype, tuple(params.shape), total))
        flat = params.detach().to(device=device).clone()
        t = {k: flat[o: o + _numel(s)].view(*s) for k, (o, s) in offsets.items()}
        layers = [(t["W0"], t["b0"])] + ([(t["W1"], t["b1"])] if L == 2 else [])
        value_layers = None
        if sd["separate_value"]:
            value_layers = [(t["V0"], t["c0"])] + ([(t["V1"], t["c1"])] if L == 2 else [])
        return cls(layers, (t["Wpi"], t["bpi"]), (t["Wv"], t["bv"]), scale.to(device), activation=sd["activation"], value_layers=value_layers)

    def to_native(self):
        """The ssg_policy record (pointers into this object's tensors: keep the policy alive while the library uses it)."""
        p = N.Policy()
        p.struct_size = C.sizeof(N.Policy)
        p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions = self.obs_dim, self.hidden, self.n_hidden_layers, self.n_actions
        p.activation = ACTIVATIONS[self.activation] | (N.POLICY_SEPARATE_VALUE if self.separate_value else 0)
        p.dev_params, p.dev_obs_scale = self.params.data_ptr(), self.obs_scale.data_ptr()
        return p

    def unpack(self):
        """{name: tensor view} of the packed buffer, by the header's offsets."""
        return {k: self.params[o: o + _numel(s)].view(*s) for k, (o, s) in self.offsets.items()}

    def forward_reference(self, obs):
        """Plain torch restatement: (x f32 [N, D], logits [N, A], value [N]) for f64 observations [N, D]."""
        torch = _torch()
        t = self.unpack()
        act = torch.tanh if self.activation == "tanh" else torch.relu
        with torch.no_grad():
            x = (obs / self.obs_scale.to(obs.device)).float()
            h = act(x @ t["W0"].T + t["b0"])
            if self.n_hidden_layers == 2:
                h = act(h @ t["W1"].T + t["b1"])
            hv = h
            if self.separate_value:
                hv = act(x @ t["V0"].T + t["c0"])
                if self.n_hidden_layers == 2:
                    hv = act(hv @ t["V1"].T + t["c1"])
            return x, h @ t["Wpi"].T + t["bpi"], (hv @ t["Wv"].T + t["bv"]).squeeze(-1)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n
