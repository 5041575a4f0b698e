"""Env surfaces over the C ABI: ``TreasureGameVec`` (N envs on one GPU, torch tensors) and
``TreasureGame`` (the N=1 drop-in for the reference ``TreasureGame``, treasure_game.py:54-114).

Seeding contract: env ``g`` of a batch created with ``seed=s,
global_offset=o`` replays, bit for bit, a reference env in a fresh process after
``random.seed(s + o + g); env = TreasureGame(); env.reset()``.  Every env owns its own
CPython-compatible MT19937 stream; the reference's envs share one process-global stream
(IM/:2, OB/:9), which is the one deliberate difference.
"""
import ctypes
import operator
import os
import random
import struct

import numpy as np
import torch

from . import _lib
from ._lib import TgError, check

OPTION_NAMES = ["go_left_option", "go_right_option", "up_ladder_option", "down_ladder_option",
                "interact_option", "down_left_option", "down_right_option", "jump_left_option",
                "jump_right_option"]  # create_options order (IM/:484-498)
STATE_NAMES = ["playerx", "playery", "handle1.angle", "handle2.angle", "key.x", "key.y",
               "bolt.locked", "goldcoin.x", "goldcoin.y"]  # get_state_descriptors (IM/:380-400)
LEVEL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "levels", "default")
# bits of a done row: the env's own end (the only bit without a step limit), and the step limit's
DONE_TERMINATED = _lib.TG_DONE_TERMINATED
DONE_TRUNCATED = _lib.TG_DONE_TRUNCATED


# ---- spaces: gym's / gymnasium's when importable, else minimal stand-ins with the same fields
def _spaces():
    for mod in ("gym.spaces", "gymnasium.spaces"):
        try:
            m = __import__(mod, fromlist=["Discrete", "Box", "MultiDiscrete"])
            return m.Discrete, m.Box, m.MultiDiscrete
        except Exception:  # noqa: BLE001 — absent or broken install: use the stand-ins
            continue

    class Discrete:
        def __init__(self, n):
            self.n = int(n)
            self.shape = ()
            self.dtype = np.int64

        def sample(self):
            return random.randrange(self.n)

        def contains(self, x):
            try:
                return 0 <= int(x) < self.n
            except (TypeError, ValueError):
                return False

        def __repr__(self):
            return "Discrete(%d)" % self.n

    class Box:
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.shape = tuple(shape)
            self.dtype = np.dtype(dtype)
            self.low = np.full(self.shape, low, self.dtype)
            self.high = np.full(self.shape, high, self.dtype)

        def sample(self):
            return np.random.uniform(self.low, self.high).astype(self.dtype)

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

        def __repr__(self):
            return "Box(%s, %s, %s, %s)" % (self.low.min(), self.high.max(), self.shape, self.dtype)

    class MultiDiscrete:
        def __init__(self, nvec):
            self.nvec = np.asarray(nvec, np.int64)
            self.shape = self.nvec.shape
            self.dtype = np.int64

        def sample(self):
            return (np.random.random_sample(self.shape) * self.nvec).astype(np.int64)

        def contains(self, x):
            x = np.asarray(x)
            return x.shape == self.shape and bool(np.all((x >= 0) & (x < self.nvec)))

        def __repr__(self):
            return "MultiDiscrete(%s)" % (self.nvec,)

    return Discrete, Box, MultiDiscrete


Discrete, Box, MultiDiscrete = _spaces()


def read_level(path=LEVEL_DIR):
    """The three level files (reference formats, IM/:75-202) as bytes."""
    out = []
    for f in ("domain.txt", "domain-objects.txt", "domain-interactions.txt"):
        with open(os.path.join(path, f), "rb") as fh:
            out.append(fh.read())
    return tuple(out)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the learned actor's parameters (tg_policy_mlp_load; include/tg_amd.h) -------------------
MLP_HIDDEN = (16, 32, 64, 128)
MLP_KEYS = ("obs_scale", "obs_shift", "w1", "b1", "w2", "b2", "wp", "bp", "wv", "bv")


def mlp_param_count(hidden):
    """Packed f32 values of a network of hidden width ``hidden``: H*H + 21*H + 28."""
    h = int(hidden)
    if h not in MLP_HIDDEN:
        raise ValueError("hidden must be one of %s (got %r)" % (MLP_HIDDEN, hidden))
    return h * h + 21 * h + 28


def _mlp_hidden_of(count):
    for h in MLP_HIDDEN:
        if mlp_param_count(h) == count:
            return h
    raise ValueError("%d values are no packed parameter array (H*H + 21*H + 28 for H in %s)"
                     % (count, MLP_HIDDEN))


def pack_mlp_params(params):
    """The actor's parameters as the one flat float32 array tg_policy_mlp_load reads:
    obs_scale[9], obs_shift[9], W1[H][9], b1[H], W2[H][H], b2[H], Wp[9][H], bp[9], Wv[H], bv[1].

    ``params``: a dict of arrays or tensors with the keys ``obs_scale, obs_shift, w1, b1, w2, b2,
    wp, bp, wv, bv``; the weights in torch's ``nn.Linear.weight`` orientation [out, in] (``wv``
    [H] or [1, H], ``bv`` a scalar or [1]).  Shapes are checked (``ValueError``).  Needs no GPU."""
    a = {}
    for k in MLP_KEYS:
        if k not in params:
            continue
        v = params[k]
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        a[k] = np.asarray(v, dtype=np.float32)
    _mlp_check_shapes(a)
    return np.concatenate([a[k].reshape(-1) for k in MLP_KEYS]).astype(np.float32)


def _mlp_check_shapes(a):
    """ValueError unless the dict holds every key with its shape; returns H"""
    missing = [k for k in MLP_KEYS if k not in a]
    if missing:
        raise ValueError("params lacks %s" % ", ".join(missing))
    w2 = tuple(a["w2"].shape)
    if len(w2) != 2 or w2[0] != w2[1]:
        raise ValueError("w2 must be [H, H] (got %s)" % (w2,))
    h = w2[0]
    if h not in MLP_HIDDEN:
        raise ValueError("hidden width %d: must be one of %s" % (h, MLP_HIDDEN))
    shapes = {"obs_scale": [(9,)], "obs_shift": [(9,)], "w1": [(h, 9)], "b1": [(h,)],
              "w2": [(h, h)], "b2": [(h,)], "wp": [(9, h)], "bp": [(9,)],
              "wv": [(h,), (1, h)], "bv": [(), (1,)]}
    for k in MLP_KEYS:
        if tuple(a[k].shape) not in shapes[k]:
            raise ValueError("%s has shape %s, expected %s (H = %d)"
                             % (k, tuple(a[k].shape), " or ".join(map(str, shapes[k])), h))
    return h


class TreasureGameVec:
    """``num_envs`` Treasure Game envs resident in one GPU's HBM.

    ``step`` takes an int32 action tensor [N] (values in [-9, 8], Python list indexing as in
    TG/:92) and returns ``(obs f64 [N,9], reward i32 [N], valid u8 [N], done u8 [N], info)``;
    ``valid == 0`` is the reference's ``None`` reward (OP/:22-23).  Returned tensors are the
    env's own output buffers and are overwritten by the next call (``copy=True`` clones).
    With ``autoreset=True`` an env that returns done is reset in the same step (the reference
    never resets by itself; this is the equivalent of calling ``reset()`` right after), its
    pre-reset obs goes to ``info["final_obs"]`` and its episode (return, length) to
    ``episodes()``.
    ``max_episode_steps`` (``set_time_limit``) truncates episodes at that many steps on the
    device, in ``step`` and inside ``rollout``: ``done`` is then a bit set, ``DONE_TERMINATED``
    (1, the only value without a limit) and ``DONE_TRUNCATED`` (2).  With auto-reset a truncated
    env is reset in the same step as a terminated one is and its episode is queued with the
    truncated flag (``episodes(truncated=True)``); without, it is only flagged, at every step
    from the limit on.
    """

    def __init__(self, num_envs, seed=0, device=None, global_offset=0, autoreset=False,
                 level_dir=None, copy=False, mode="compact", max_episode_steps=None):
        if not torch.cuda.is_available():
            raise TgError("TreasureGameVec needs a ROCm GPU (gfx950); there is no CPU path")
        self._L = _lib.load()
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(num_envs)
        self.seed = int(seed)
        self.global_offset = int(global_offset)
        if self.num_envs <= 0 or self.global_offset < 0:
            raise ValueError("num_envs must be > 0 and global_offset >= 0")
        # env g is random.seed(seed + global_offset + g); the device seeds init_by_array with
        # a key of at most two 32-bit words, so every env's seed must lie in [0, 2^64)
        # (CPython's abs() of a negative seed is not monotone in g: TreasureGame maps it)
        if self.seed < 0 or self.seed + self.global_offset + self.num_envs - 1 >= 2**64:
            raise ValueError("seed + global_offset + g must lie in [0, 2**64) for every env "
                             "(got seed=%d, global_offset=%d, num_envs=%d)"
                             % (self.seed, self.global_offset, self.num_envs))
        self.autoreset = bool(autoreset)
        self.copy = bool(copy)
        texts = read_level(level_dir) if level_dir else (None, None, None)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self._L.tg_create(ctypes.byref(h), self.num_envs, self.seed,
                                    self.global_offset, self.device.index, *texts), "tg_create")
        self._h = h
        n, dev = self.num_envs, self.device
        self._obs = torch.empty((n, 9), dtype=torch.float64, device=dev)
        self._final = torch.empty((n, 9), dtype=torch.float64, device=dev) if autoreset else None
        self._rew = torch.empty(n, dtype=torch.int32, device=dev)
        self._valid = torch.empty(n, dtype=torch.uint8, device=dev)
        self._done = torch.empty(n, dtype=torch.uint8, device=dev)
        self._act = torch.empty(n, dtype=torch.int32, device=dev)
        self._mask = torch.empty(n, dtype=torch.int16, device=dev)
        self.action_space = Discrete(_lib.NUM_ACTIONS)
        self.observation_space = Box(np.float32(0.0), np.float32(1.0), shape=(_lib.OBS_DIM,))
        self.option_names = list(OPTION_NAMES)
        self._mode = "compact"
        if mode != "compact":
            self.set_mode(mode)
        self.max_episode_steps = None
        if max_episode_steps is not None:
            self.set_time_limit(max_episode_steps)

    # -- plumbing ---------------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _out(self, t):
        return t.clone() if self.copy else t

    @property
    def handle(self):
        if self._h is None:
            raise TgError("env is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.device)
            for s in list(getattr(self, "_snaps", ())):
                s.close()
            self._L.tg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter teardown
            pass

    # -- reference surface --------------------------------------------------------------------
    def reset(self, mask=None):
        """reset() (TG/:78-81) of every env, or of those with mask[i] != 0."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            if m.numel() != self.num_envs:
                raise ValueError("mask must have num_envs entries")
        check(self._L.tg_reset(self.handle, _ptr(m), _ptr(self._obs), self._stream()), "tg_reset")
        return self._out(self._obs)

    def step(self, actions):
        """step(a) (TG/:91-96) for every env."""
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.int32 and a.device == self.device
                and a.is_contiguous()):
            a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        if a.numel() != self.num_envs:
            raise ValueError("actions must have num_envs entries")
        check(self._L.tg_step(self.handle, _ptr(a), _ptr(self._obs), _ptr(self._rew),
                              _ptr(self._valid), _ptr(self._done), _ptr(self._final),
                              _lib.TG_STEP_AUTORESET if self.autoreset else 0, self._stream()),
              "tg_step")
        info = {"final_obs": self._out(self._final)} if self.autoreset else {}
        return (self._out(self._obs), self._out(self._rew), self._out(self._valid),
                self._out(self._done), info)

    def rollout(self, steps, t0=0, action_seed=0x5EED0001, policy="uniform", obs=True,
                actions=True, check_flow=True, gae=None):
        """``steps`` env-steps in one call with the on-device synthetic policy (tg_rollout):
        step t0 + s takes ``policy_actions(t0 + s, action_seed, policy)``, evaluated inside the
        step kernels.  Returns step-major device tensors: reward i32 [K, N], valid / done u8
        [K, N], and (optionally) obs f64 [K, N, 9], actions i32 [K, N].  With auto-reset the
        obs rows are the post-reset ones and finished episodes queue for ``episodes()``.

        ``policy="mlp"`` / ``"mlp_greedy"``: the learned actor of ``set_policy_mlp`` instead
        (tg_rollout_mlp: per step the actor kernel, then the step kernels), which also returns
        "logp" and "value" f32 [K, N]; not in "flow" mode.

        ``gae=(gamma, lam)`` with one of the mlp policies (tg_rollout_mlp_gae): also "adv", "ret"
        and "vnext" f32 [K, N] and "vboot" f32 [N], the advantages of include/tg_amd.h's
        definition with the actor's value of every env after the last step as the bootstrap
        and, with auto-reset and a step limit, of every truncated env's pre-reset state.  The
        other outputs and the state the call leaves are unchanged by it.

        In "flow" mode a k_flow launch that fails its protocol checks (a wait past its bound,
        a sub-problem left unstepped, an item out of range) sets TG_ERR_FLOW and its rows are
        not valid: with ``check_flow`` (the default) the call then synchronises on
        ``errors()`` and raises TgError."""
        k, n, dev = int(steps), self.num_envs, self.device
        if self._mode == "flow" and self.max_episode_steps is not None:
            raise TgError("rollout() in the flow mode cannot apply max_episode_steps (k_flow has "
                          "no step boundary): use the compact or direct mode, or step()")
        out = {"reward": torch.empty((k, n), dtype=torch.int32, device=dev),
               "valid": torch.empty((k, n), dtype=torch.uint8, device=dev),
               "done": torch.empty((k, n), dtype=torch.uint8, device=dev)}
        if obs:
            out["obs"] = torch.empty((k, n, 9), dtype=torch.float64, device=dev)
        if actions:
            out["actions"] = torch.empty((k, n), dtype=torch.int32, device=dev)
        if gae is not None and policy not in ("mlp", "mlp_greedy"):
            raise TgError("rollout(gae=...) needs policy='mlp' or 'mlp_greedy' (the advantages use "
                          "the learned actor's value); gae() takes any rollout's rows")
        if policy in ("mlp", "mlp_greedy"):
            # the learned actor (set_policy_mlp) as the policy: also "logp" and "value" f32 [K, N];
            # the row the policy saw at step s is obs[s - 1] (observe() before the call for s = 0)
            if self._mode == "flow":
                raise TgError("rollout(policy=%r) needs the compact or direct mode (k_flow "
                              "evaluates its policy inside the kernel)" % policy)
            out["logp"] = torch.empty((k, n), dtype=torch.float32, device=dev)
            out["value"] = torch.empty((k, n), dtype=torch.float32, device=dev)
            mlp_mode = _lib.TG_MLP_GREEDY if policy == "mlp_greedy" else _lib.TG_MLP_SAMPLE
            if gae is not None:
                gamma, lam = gae
                for key in ("adv", "ret", "vnext"):
                    out[key] = torch.empty((k, n), dtype=torch.float32, device=dev)
                out["vboot"] = torch.empty(n, dtype=torch.float32, device=dev)
                check(self._L.tg_rollout_mlp_gae(
                    self.handle, k, action_seed, int(t0), mlp_mode,
                    _lib.TG_STEP_AUTORESET if self.autoreset else 0, _ptr(out.get("actions")),
                    _ptr(out.get("obs")), _ptr(out["reward"]), _ptr(out["valid"]),
                    _ptr(out["done"]), _ptr(out["logp"]), _ptr(out["value"]), float(gamma),
                    float(lam), _ptr(out["adv"]), _ptr(out["ret"]), _ptr(out["vnext"]),
                    _ptr(out["vboot"]), self._stream()), "tg_rollout_mlp_gae")
                return out
            check(self._L.tg_rollout_mlp(
                self.handle, k, action_seed, int(t0), mlp_mode,
                _lib.TG_STEP_AUTORESET if self.autoreset else 0, _ptr(out.get("actions")),
                _ptr(out.get("obs")), _ptr(out["reward"]), _ptr(out["valid"]), _ptr(out["done"]),
                _ptr(out["logp"]), _ptr(out["value"]), self._stream()), "tg_rollout_mlp")
            return out
        pol = {"uniform": _lib.TG_POLICY_UNIFORM, "masked": _lib.TG_POLICY_MASKED}[policy]
        check(self._L.tg_rollout(self.handle, k, action_seed, int(t0), pol,
                                 _lib.TG_STEP_AUTORESET if self.autoreset else 0,
                                 _ptr(out.get("actions")), _ptr(out.get("obs")),
                                 _ptr(out["reward"]), _ptr(out["valid"]), _ptr(out["done"]),
                                 self._stream()), "tg_rollout")
        if check_flow and self._mode == "flow" and self.errors() & _lib.TG_ERR_FLOW:
            raise TgError("tg_rollout: a k_flow launch set TG_ERR_FLOW (its rows are not valid)")
        return out

    def gae(self, reward, done, value, vboot, gamma, lam, vnext=None):
        """Advantages of any rollout's step-major rows (tg_gae; the definition:
        include/tg_amd.h): ``reward`` i32, ``done`` u8, ``value`` f32 [K, N] and ``vboot`` f32
        [N] (the value of every env's state after the last step), contiguous tensors on the
        env's device.  ``vnext`` f32 [K, N]: its entries where ``done`` is DONE_TRUNCATED alone
        are read as the value of the truncated env's pre-reset state (a step() loop gets them
        from ``final_obs``); None: a truncated env's next value is ``value[s + 1]`` (``vboot``
        after the last step).  Returns ``{"adv", "ret", "vnext"}`` f32 [K, N]; a given
        ``vnext`` is completed in place."""
        n, dev = self.num_envs, self.device
        if not (isinstance(reward, torch.Tensor) and reward.dim() == 2 and reward.shape[1] == n):
            raise ValueError("reward must be a [K, num_envs] tensor")
        k = int(reward.shape[0])
        want = {"reward": (reward, (k, n), torch.int32), "done": (done, (k, n), torch.uint8),
                "value": (value, (k, n), torch.float32), "vboot": (vboot, (n,), torch.float32)}
        if vnext is not None:
            want["vnext"] = (vnext, (k, n), torch.float32)
        for name, (t, shape, dt) in want.items():
            if not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == shape
                    and t.is_contiguous() and t.device == dev):
                raise ValueError("%s must be a contiguous %s tensor of shape %s on %s"
                                 % (name, dt, shape, dev))
        out = {"adv": torch.empty((k, n), dtype=torch.float32, device=dev),
               "ret": torch.empty((k, n), dtype=torch.float32, device=dev),
               "vnext": vnext if vnext is not None
               else torch.empty((k, n), dtype=torch.float32, device=dev)}
        check(self._L.tg_gae(self.handle, k, float(gamma), float(lam), _ptr(reward), _ptr(done),
                             _ptr(value), _ptr(out["vnext"]), _ptr(vboot),
                             0 if vnext is None else 1, _ptr(out["adv"]), _ptr(out["ret"]),
                             self._stream()), "tg_gae")
        return out

    def set_groups(self, groups=1, stagger=False):
        """rollout() steps the batch as ``groups`` contiguous groups, each on a stream of its
        own (tg_set_groups: overlaps one group's option loops with another's bandwidth-bound
        passes; results identical).  1: off."""
        check(self._L.tg_set_groups(self.handle, int(groups), 1 if stagger else 0),
              "tg_set_groups")

    def available_mask(self):
        """available_mask (TG/:83-89) as bits: int16 [N], bit k == option k can run."""
        check(self._L.tg_available_mask(self.handle, _ptr(self._mask), self._stream()),
              "tg_available_mask")
        return self._out(self._mask)

    def observe(self):
        """get_state (IM/:368-378) of every env."""
        check(self._L.tg_observe(self.handle, _ptr(self._obs), self._stream()), "tg_observe")
        return self._out(self._obs)

    # -- batch extras -------------------------------------------------------------------------
    def policy_actions(self, t, action_seed=0x5EED0001, policy="uniform", out=None):
        """Counter-hash synthetic actions for step t (bench / parity), keyed by GLOBAL env id."""
        pol = {"uniform": _lib.TG_POLICY_UNIFORM, "masked": _lib.TG_POLICY_MASKED}[policy]
        out = self._act if out is None else out
        check(self._L.tg_policy_actions(self.handle, action_seed, int(t), pol, _ptr(out),
                                        self._stream()), "tg_policy_actions")
        return out

    def set_policy_mlp(self, params, act="tanh", masked=True):
        """Load the learned actor (tg_policy_mlp_load): a two-hidden-layer MLP over the obs row
        with a 9-way policy head and a value head (the arithmetic: include/tg_amd.h).

        ``params``: the dict ``pack_mlp_params`` takes, or an already packed float32 array /
        tensor (a device tensor is used in place).  The copy into the handle's buffer is
        queued on the current stream, so weights can be refreshed between rollouts without a
        synchronisation.  ``masked``: sample among the options ``available_mask`` allows."""
        a = {"relu": _lib.TG_ACT_RELU, "tanh": _lib.TG_ACT_TANH}[act]
        if isinstance(params, dict):
            if all(isinstance(v, torch.Tensor) and v.device == self.device
                   for v in params.values()):  # a module's tensors: packed on the device
                _mlp_check_shapes(params)
                params = torch.cat([params[k].detach().reshape(-1).to(torch.float32)
                                    for k in MLP_KEYS])
            else:
                params = pack_mlp_params(params)
        p = torch.as_tensor(params)
        if p.dtype != torch.float32 or p.dim() != 1:
            raise ValueError("packed parameters must be a flat float32 array")
        hidden = _mlp_hidden_of(p.numel())
        p = p.to(self.device).contiguous()
        check(self._L.tg_policy_mlp_load(self.handle, hidden, a, 1 if masked else 0, _ptr(p),
                                         self._stream()), "tg_policy_mlp_load")
        self.mlp_hidden = hidden

    def policy_mlp(self, t, action_seed=0x5EED0001, greedy=False, logits=False, out=None):
        """The learned actor on every env's current state for step ``t`` (tg_policy_mlp):
        ``(actions i32 [N], logp f32 [N], value f32 [N])`` and, with ``logits``, the policy
        head's f32 [N, 9].  Sampling is keyed by (action_seed, GLOBAL env id, t); ``greedy``
        takes the allowed argmax.  The tensors are the env's own buffers, overwritten by the
        next call, unless ``out`` gives some ({"actions", "logp", "value", "logits"}: contiguous
        device tensors of exactly those shapes and dtypes)."""
        n, dev = self.num_envs, self.device
        want = {"actions": ((n,), torch.int32), "logp": ((n,), torch.float32),
                "value": ((n,), torch.float32), "logits": ((n, 9), torch.float32)}
        bufs = {}
        for k, (shape, dt) in want.items():
            if k == "logits" and not logits:
                continue
            b = None if out is None else out.get(k)
            if b is None:
                own = getattr(self, "_mlp_out", None)
                if own is None:
                    own = self._mlp_out = {}
                if k not in own:
                    own[k] = torch.empty(shape, dtype=dt, device=dev)
                b = own[k]
            elif not (isinstance(b, torch.Tensor) and b.dtype == dt and tuple(b.shape) == shape
                      and b.is_contiguous() and b.device == dev):
                raise ValueError("out[%r] must be a contiguous %s tensor of shape %s on %s"
                                 % (k, dt, shape, dev))
            bufs[k] = b
        check(self._L.tg_policy_mlp(self.handle, action_seed, int(t),
                                    _lib.TG_MLP_GREEDY if greedy else _lib.TG_MLP_SAMPLE,
                                    _ptr(bufs["actions"]), _ptr(bufs["logp"]), _ptr(bufs["value"]),
                                    _ptr(bufs.get("logits")), self._stream()), "tg_policy_mlp")
        res = (bufs["actions"], bufs["logp"], bufs["value"])
        return res + (bufs["logits"],) if logits else res

    def drain_episodes(self, out, count):
        """Asynchronous device drain: up to out.shape[0] records -> ``out`` (int64 [cap, 2],
        the raw 16-B tg_episode rows), their number -> ``count`` (int32 [1])."""
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.int64 and out.dim() == 2
                and out.size(1) == 2 and out.is_contiguous() and out.device == self.device):
            raise ValueError("out must be a contiguous int64 [cap, 2] tensor on %s" % self.device)
        if not (isinstance(count, torch.Tensor) and count.dtype == torch.int32
                and count.numel() >= 1 and count.is_contiguous() and count.device == self.device):
            raise ValueError("count must be a contiguous int32 tensor of >= 1 element on %s"
                             % self.device)
        if out.size(0) >= 2**31:
            raise ValueError("out holds too many rows")
        check(self._L.tg_episodes(self.handle, _ptr(out), _ptr(count), out.shape[0],
                                  self._stream()), "tg_episodes")

    @staticmethod
    def decode_episodes(rows, truncated=False):
        """raw tg_episode rows (int64 [k, 2]) -> int64 [k, 3] = (env, return, length), the step
        limit's flag stripped from the length; ``truncated=True``: [k, 4], the last column 1 for
        an episode the step limit ended."""
        packed = rows[:, 1]
        ret = ((packed & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000  # sign-extend the i32 half
        ln = packed >> 32
        cols = [rows[:, 0], ret, ln & (_lib.TG_EPISODE_TRUNCATED - 1)]
        if truncated:
            cols.append(((ln & _lib.TG_EPISODE_TRUNCATED) != 0).to(torch.int64))
        return torch.stack(cols, dim=1)

    def episodes(self, cap=None, truncated=False):
        """Completed (auto-reset) episodes, oldest first, up to ``cap`` of them:
        int64 [k, 3] = (global env, return, length) on the device (synchronises);
        ``truncated=True`` adds a column, 1 for an episode the step limit ended."""
        cap = self.num_envs if cap is None else int(cap)
        rec = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.drain_episodes(rec[:cap], cnt)
        return self.decode_episodes(rec[: int(cnt.item())], truncated)

    def errors(self):
        v = ctypes.c_uint32(0)
        check(self._L.tg_errors(self.handle, ctypes.byref(v), self._stream()), "tg_errors")
        return int(v.value)

    def set_serve(self, on=True):
        """A 1-env handle's N = 1 calls (TreasureGame.step / reset) through the resident server
        kernel (the default; tg_set_serve) or one launch + synchronisation each: identical
        results, the server without the launch and the synchronisation."""
        check(self._L.tg_set_serve(self.handle, 1 if on else 0), "tg_set_serve")

    def set_mode(self, mode="compact", run_blocks=0):
        """Step implementation: "compact" (two-pass, default), "direct" (one lane per env
        runs in place) or "flow" (as compact per step; rollout() runs up to 16 steps per launch,
        chunks advancing without a batch-wide barrier between steps); all bit-identical."""
        m = {"direct": _lib.TG_MODE_DIRECT, "compact": _lib.TG_MODE_COMPACT,
             "flow": _lib.TG_MODE_FLOW}[mode]
        check(self._L.tg_set_mode(self.handle, m, int(run_blocks)), "tg_set_mode")
        self._mode = mode

    def set_time_limit(self, max_episode_steps):
        """Truncate episodes at ``max_episode_steps`` steps on the device, from the next step
        on (tg_set_time_limit); None or 0: off.  An episode already that long is truncated by
        the next step."""
        m = 0 if max_episode_steps is None else int(max_episode_steps)
        check(self._L.tg_set_time_limit(self.handle, m), "tg_set_time_limit")
        self.max_episode_steps = m or None

    def set_episode_capacity(self, cap):
        """Resize the completed-episode queue (discards what it holds)."""
        check(self._L.tg_set_episode_capacity(self.handle, int(cap)), "tg_set_episode_capacity")

    def predicate_table(self, x0, x1, y0, y1, door_bits):
        """The six collision predicates (IM/:232-288) evaluated on the device at every pixel
        of [x0, x1) x [y0, y1) with doors closed per door_bits: uint8 [y1-y0, x1-x0] device
        tensor, bit k = up_clear, can_go_up, can_go_down, can_go_left, can_go_right, can_fall."""
        out = torch.empty((y1 - y0, x1 - x0), dtype=torch.uint8, device=self.device)
        check(self._L.tg_predicate_table(self.handle, x0, x1, y0, y1, int(door_bits), _ptr(out),
                                         self._stream()), "tg_predicate_table")
        return out

    def set_timing(self, every=1):
        """HIP-event timing of every ``every``-th step launch (0 / False: off; True: every
        launch).  stats() then holds kernel_ms / run_ms summed over timed_launches."""
        check(self._L.tg_set_timing(self.handle, int(every)), "tg_set_timing")

    def regenerate(self):
        """Regenerate every stale MT half still queued (tg_regenerate: results never depend on
        it; a timed loop calls it at its end so that it holds its own steps' regeneration)."""
        check(self._L.tg_regenerate(self.handle, self._stream()), "tg_regenerate")

    def stats(self):
        """tg_stats as a dict (include/tg_amd.h): counters since creation / ``stats_reset()``,
        among them ``regens`` (MT generations regenerated, by whichever kernel) and
        ``regens_quiet`` (of those, the ones k_run's chunk-less waves regenerated in the step
        that listed them)."""
        s = _lib.Stats()
        check(self._L.tg_get_stats(self.handle, ctypes.byref(s)), "tg_get_stats")
        return s.as_dict()

    def stats_reset(self):
        check(self._L.tg_stats_reset(self.handle), "tg_stats_reset")

    def kernel_info(self):
        """{kernel: (workgroups per CU, VGPRs, LDS bytes)} of the step kernels (tg_kernel_info)"""
        out = {}
        for name, k in (("k_classify", 0), ("k_run", 1), ("k_regen", 2)):
            v = [ctypes.c_int32() for _ in range(4)]
            check(self._L.tg_kernel_info(self.handle, k, *[ctypes.byref(x) for x in v]),
                  "tg_kernel_info")
            out[name] = {"blocks_per_cu": v[0].value, "waves_per_simd": v[0].value,
                         "vgprs": v[1].value, "lds_bytes": v[3].value}
        return out

    # -- render('rgb_array') (TG/:98-105; DR/ draw_domain) ---------------------------------------
    def render_init(self, sprites=None):
        """Load the sprite sheet (uint8 [24, h, w, 4] RGBA, ``render.load_sprites`` /
        ``render.synthetic_sprites``; default: the installed reference's sprites)."""
        from . import render as R
        if sprites is None:
            sprites = R.load_sprites()
        sheet = np.ascontiguousarray(sprites, np.uint8)
        if sheet.ndim != 4 or sheet.shape[0] != _lib.TG_SPR_COUNT or sheet.shape[3] != 4:
            raise ValueError("sprite sheet must be uint8 [%d, h, w, 4]" % _lib.TG_SPR_COUNT)
        check(self._L.tg_render_init(self.handle, sheet.ctypes.data_as(ctypes.c_void_p),
                                     sheet.shape[2], sheet.shape[1]), "tg_render_init")
        h, w = ctypes.c_int32(), ctypes.c_int32()
        check(self._L.tg_frame_shape(self.handle, ctypes.byref(h), ctypes.byref(w)),
              "tg_frame_shape")
        self.frame_shape = (h.value, w.value, 3)

    def frame_shape_scaled(self, scale=8, gray=False):
        """(h, w, c) of ``render(scale=scale, gray=gray)``'s frames: (78, 84, 3) for the default
        level at scale 8.  ``scale`` must divide 48 (``TgError`` otherwise)."""
        h, w = ctypes.c_int32(), ctypes.c_int32()
        check(self._L.tg_frame_shape_scaled(self.handle, int(scale), ctypes.byref(h),
                                            ctypes.byref(w)), "tg_frame_shape_scaled")
        return (h.value, w.value, 1 if gray else 3)

    def _render_scaled(self, first, count, out, scale, gray):
        if getattr(self, "frame_shape", None) is None:
            self.render_init()
        count = self.num_envs - first if count is None else int(count)
        shape = self.frame_shape_scaled(scale, gray)
        if out is None:
            out = torch.empty((max(count, 0),) + shape, dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device
              or tuple(out.shape) != (count,) + shape):
            raise ValueError("out must be a contiguous uint8 [%d, %d, %d, %d] tensor on %s"
                             % ((count,) + shape + (self.device,)))
        check(self._L.tg_render_scaled(self.handle, int(first), count, int(scale), shape[2],
                                       _ptr(out), self._stream()), "tg_render_scaled")
        return out

    def frame_shape_view(self, radius, scale=1, gray=False):
        """(h, w, c) of ``render(view=radius, scale=scale, gray=gray)``'s frames, h = w =
        48 * (2 * radius + 1) / scale: (18, 18, 1) at radius 1, scale 8, gray.  ``radius`` must
        be 1..7 and ``scale`` divide 48 (``TgError`` otherwise)."""
        h, w = ctypes.c_int32(), ctypes.c_int32()
        check(self._L.tg_frame_shape_view(self.handle, int(radius), int(scale), ctypes.byref(h),
                                          ctypes.byref(w)), "tg_frame_shape_view")
        return (h.value, w.value, 1 if gray else 3)

    def _render_view(self, first, count, out, scale, gray, view, origin):
        if getattr(self, "frame_shape", None) is None:
            self.render_init()
        count = self.num_envs - first if count is None else int(count)
        shape = self.frame_shape_view(view, scale, gray)
        if out is None:
            out = torch.empty((max(count, 0),) + shape, dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device
              or tuple(out.shape) != (count,) + shape):
            raise ValueError("out must be a contiguous uint8 [%d, %d, %d, %d] tensor on %s"
                             % ((count,) + shape + (self.device,)))
        if origin is not None and (origin.dtype != torch.int32 or not origin.is_contiguous()
                                   or origin.device != self.device
                                   or tuple(origin.shape) != (count, 2)):
            raise ValueError("origin must be a contiguous int32 [%d, 2] tensor on %s"
                             % (count, self.device))
        check(self._L.tg_render_view(self.handle, int(first), count, int(view), int(scale),
                                     shape[2], _ptr(out), None if origin is None else _ptr(origin),
                                     self._stream()), "tg_render_view")
        return out

    def render(self, first=0, count=None, out=None, scale=1, gray=False, view=None, origin=None):
        """render('rgb_array') of envs [first, first+count): uint8 [count, H*48, W*48, 3]
        on the device (the reference's ``rgb`` array per env, TG/:103-105).

        ``scale`` (a divisor of 48) and ``gray`` give the pixel-observation form instead,
        uint8 [count, H*48/scale, W*48/scale, 3 or 1]: the full frame average-pooled over
        scale x scale boxes (halves round up), then (77 R + 150 G + 29 B + 128) >> 8 for gray,
        rendered directly at that size (tg_render_scaled).  The first call for a scale builds
        its tables and synchronises.

        ``view=r`` (1..7) gives the agent-centred window instead (tg_render_view): the
        (2r+1) x (2r+1) cells around the hero's cell (px // 48, (py + 24) // 48), uint8
        [count, n, n, 3 or 1] with n = 48 * (2r+1) / scale, the zero-padded crop of the frame
        ``scale`` and ``gray`` select.  ``origin``, an int32 [count, 2] device tensor, receives
        each window's origin (ox, oy) in cells."""
        if view is not None:
            return self._render_view(first, count, out, scale, gray, view, origin)
        if origin is not None:
            raise ValueError("origin is the window's: pass view=radius with it")
        if scale != 1 or gray:
            return self._render_scaled(first, count, out, scale, gray)
        if getattr(self, "frame_shape", None) is None:
            self.render_init()
        count = self.num_envs - first if count is None else int(count)
        if out is None:
            out = torch.empty((count,) + self.frame_shape, dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device
              or tuple(out.shape) != (count,) + self.frame_shape):
            raise ValueError("out must be a contiguous uint8 [%d, %d, %d, 3] tensor on %s"
                             % ((count,) + self.frame_shape[:2] + (self.device,)))
        check(self._L.tg_render(self.handle, int(first), count, _ptr(out), self._stream()),
              "tg_render")
        return out

    STATE_KEYS = ("pos", "flags", "objs", "ang", "mt", "mt_pos", "ep")

    def read_state(self, mt=False):
        """Host copy of the SoA state (checkpoints / tests); ``mt=True`` adds each env's
        ``random.getstate()`` equivalent (624 MT words + index)."""
        n = self.num_envs
        out = {"pos": np.zeros((n, 2), np.int32), "flags": np.zeros(n, np.uint32),
               "objs": np.zeros((n, 4), np.int32), "ang": np.zeros((n, 2), np.float64),
               "mt_pos": np.zeros(n, np.uint32), "ep": np.zeros((n, 2), np.int32)}
        if mt:
            out["mt"] = np.zeros((n, 624), np.uint32)

        def p(k):
            return out[k].ctypes.data_as(ctypes.c_void_p) if k in out else None

        check(self._L.tg_read_state(self.handle, *[p(k) for k in self.STATE_KEYS]),
              "tg_read_state")
        return out

    def write_state(self, state):
        """Restore a ``read_state(mt=True)`` snapshot (same num_envs): every env continues
        bit-exactly from it."""
        n = self.num_envs
        shapes = {"pos": (n, 2), "flags": (n,), "objs": (n, 4), "ang": (n, 2), "mt": (n, 624),
                  "mt_pos": (n,), "ep": (n, 2)}
        dt = {"pos": np.int32, "flags": np.uint32, "objs": np.int32, "ang": np.float64,
              "mt": np.uint32, "mt_pos": np.uint32, "ep": np.int32}
        arrs = {}
        for k in self.STATE_KEYS:
            if k not in state:
                if k == "ep":
                    continue
                raise KeyError("state lacks %r (use read_state(mt=True))" % k)
            a = np.ascontiguousarray(state[k], dt[k])
            if a.shape != shapes[k]:
                raise ValueError("state[%r] has shape %s, expected %s" % (k, a.shape, shapes[k]))
            arrs[k] = a
        # (no synchronisation here: tg_write_state stops a resident N = 1 server first and
        # synchronises the device itself before it writes; waiting here would wait for that
        # server to leave by its idle limit)
        check(self._L.tg_write_state(self.handle, *[arrs[k].ctypes.data_as(ctypes.c_void_p)
                                                    if k in arrs else None
                                                    for k in self.STATE_KEYS]), "tg_write_state")

    def save(self, path):
        """Checkpoint every env's state (np.savez)."""
        np.savez(path, **self.read_state(mt=True))

    def load(self, path):
        """Resume from a ``save`` checkpoint."""
        with np.load(path) as z:
            self.write_state({k: z[k] for k in z.files})

    # -- device-resident snapshots ----------------------------------------------------------------
    def snapshot(self, slots):
        """A ``Snapshot`` of ``slots`` saved envs in device memory (tg_snap_create): the
        reference's ``copy.deepcopy(env)`` for subsets of the batch, without a host copy or a
        synchronisation.  Closed with the env if not before."""
        return Snapshot(self, slots)

    def _index(self, x, what):
        """an index argument as a contiguous int64 tensor on the env's device (converted once)"""
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.int64 and x.device == self.device
                and x.is_contiguous()):
            x = torch.as_tensor(x, device=self.device).to(torch.int64).contiguous()
        if x.dim() != 1:
            raise ValueError("%s must be one-dimensional" % what)
        return x

    def fork(self, src, dst, seeds=None):
        """Env ``dst[k]`` becomes a copy of env ``src[k]`` (``copy.deepcopy``; with ``seeds``,
        followed by ``random.seed(seeds[k])``): one save and one load through a scratch snapshot
        the env keeps, so every source is read before any env is written and ``dst`` may overlap
        ``src``.  A source may be named any number of times (fan-out).  On the current stream,
        no synchronisation once the scratch is large enough."""
        src, dst = self._index(src, "src"), self._index(dst, "dst")
        k = src.numel()
        if dst.numel() != k:
            raise ValueError("src and dst must have the same number of entries")
        if k == 0:
            return
        scratch = getattr(self, "_fork_snap", None)
        if scratch is None or scratch._s is None or len(scratch) < k:
            if scratch is not None:
                scratch.close()
            self._fork_snap = scratch = Snapshot(self, max(k, 64))
            self._fork_slots = torch.arange(len(scratch), dtype=torch.int64, device=self.device)
        slots = self._fork_slots[:k]
        scratch.save(src, slots)
        scratch.load(slots, dst, seeds)


class Snapshot:
    """``slots`` saved envs of one ``TreasureGameVec`` in device memory (tg_snap_*): ``save``
    copies envs into slots and ``load`` slots into envs, through index tensors on the env's
    device, as kernels on the current stream (no host copy, no synchronisation).  ``read`` and
    ``write`` move slots to and from the host in ``read_state(mt=True)``'s format, so an archive
    can outlive the env.  Index arguments are int64 tensors; anything else is converted once."""

    def __init__(self, vec, slots):
        self._vec = vec
        self._s = None
        s = ctypes.c_void_p()
        check(vec._L.tg_snap_create(vec.handle, int(slots), ctypes.byref(s)), "tg_snap_create")
        self._s = s
        self._slots = int(vec._L.tg_snap_slots(s))
        if not hasattr(vec, "_snaps"):
            vec._snaps = []
        vec._snaps.append(self)

    def __len__(self):
        return self._slots

    @property
    def handle(self):
        if self._s is None:
            raise TgError("snapshot is closed")
        return self._s

    def close(self):
        if getattr(self, "_s", None) is not None:
            if self._vec._h is not None:  # (tg_destroy frees a handle's snapshots itself)
                self._vec._L.tg_snap_destroy(self._s)
            self._s = None
            if self in self._vec._snaps:
                self._vec._snaps.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter teardown
            pass

    def save(self, envs, slots):
        """slot ``slots[k]`` <- env ``envs[k]`` as it is at this point of the stream"""
        v = self._vec
        envs, slots = v._index(envs, "envs"), v._index(slots, "slots")
        if envs.numel() != slots.numel():
            raise ValueError("envs and slots must have the same number of entries")
        check(v._L.tg_snap_save(v.handle, self.handle, _ptr(envs), _ptr(slots), envs.numel(),
                                v._stream()), "tg_snap_save")

    def load(self, slots, envs, seeds=None):
        """env ``envs[k]`` <- slot ``slots[k]``; with ``seeds`` (uint64, or int64 reinterpreted)
        the env keeps the slot's game state and takes the stream of ``random.seed(seeds[k])``"""
        v = self._vec
        envs, slots = v._index(envs, "envs"), v._index(slots, "slots")
        if envs.numel() != slots.numel():
            raise ValueError("slots and envs must have the same number of entries")
        if seeds is not None:
            if not (isinstance(seeds, torch.Tensor) and seeds.dtype in (torch.int64, torch.uint64)):
                seeds = torch.from_numpy(np.ascontiguousarray(
                    np.asarray(seeds.cpu() if isinstance(seeds, torch.Tensor) else seeds)
                    .astype(np.uint64)).view(np.int64))
            seeds = seeds.to(v.device).contiguous()
            if seeds.dim() != 1 or seeds.numel() != envs.numel():
                raise ValueError("seeds must have one entry per env")
        check(v._L.tg_snap_load(v.handle, self.handle, _ptr(slots), _ptr(envs), _ptr(seeds),
                                envs.numel(), v._stream()), "tg_snap_load")

    def _range(self, first, count):
        first = int(first)
        count = self._slots - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self._slots:
            raise ValueError("slots [%d, %d) of %d" % (first, first + count, self._slots))
        return first, count

    def read(self, first=0, count=None):
        """slots [first, first + count) as a ``read_state(mt=True)``-style dict (synchronises);
        ``mt_pos`` is what was saved (0..622) or written (0..624)"""
        first, n = self._range(first, count)
        out = {"pos": np.zeros((n, 2), np.int32), "flags": np.zeros(n, np.uint32),
               "objs": np.zeros((n, 4), np.int32), "ang": np.zeros((n, 2), np.float64),
               "mt": np.zeros((n, 624), np.uint32), "mt_pos": np.zeros(n, np.uint32),
               "ep": np.zeros((n, 2), np.int32)}
        check(self._vec._L.tg_snap_read(self.handle, first, n,
                                        *[out[k].ctypes.data_as(ctypes.c_void_p)
                                          for k in TreasureGameVec.STATE_KEYS]), "tg_snap_read")
        return out

    def write(self, state, first=0):
        """a ``read_state(mt=True)``-style dict of k envs into slots [first, first + k)
        (synchronises); validated as ``write_state`` validates, and a rejected write changes
        nothing"""
        if "flags" not in state:
            raise KeyError("state lacks 'flags' (use read_state(mt=True))")
        n = int(np.asarray(state["flags"]).shape[0])
        first, n = self._range(first, n)
        shapes = {"pos": (n, 2), "flags": (n,), "objs": (n, 4), "ang": (n, 2), "mt": (n, 624),
                  "mt_pos": (n,), "ep": (n, 2)}
        dt = {"pos": np.int32, "flags": np.uint32, "objs": np.int32, "ang": np.float64,
              "mt": np.uint32, "mt_pos": np.uint32, "ep": np.int32}
        arrs = {}
        for k in TreasureGameVec.STATE_KEYS:
            if k not in state:
                if k == "ep":
                    continue
                raise KeyError("state lacks %r (use read_state(mt=True))" % k)
            a = np.ascontiguousarray(state[k], dt[k])
            if a.shape != shapes[k]:
                raise ValueError("state[%r] has shape %s, expected %s" % (k, a.shape, shapes[k]))
            arrs[k] = a
        check(self._vec._L.tg_snap_write(self.handle, first, n,
                                         *[arrs[k].ctypes.data_as(ctypes.c_void_p)
                                           if k in arrs else None
                                           for k in TreasureGameVec.STATE_KEYS]), "tg_snap_write")


class GpuOption:
    """One entry of ``TreasureGame.option_list``: the reference's option object
    (``_Option`` / ``*_option``, _option.py:8-36, _move_options.py; create_options,
    _treasure_game_impl.py:484-498) for an env that lives on the GPU.

    ``can_run()`` is the device's ``can_run`` of this option for the env's current state, and
    ``run()`` runs it to completion on the device, exactly as ``TreasureGame.step(k)`` does
    (``option_list[k].run()``, TG/:91-96): it returns the summed tick rewards, or ``None``
    when the option cannot run (OP/:20-23).  ``done`` is True after a run, as in the reference.
    The per-tick ``policy_step`` is not exposed: the option's loop runs inside one kernel."""

    def __init__(self, env, k):
        self._env = env
        self.index = k
        self.name = OPTION_NAMES[k]
        self.done = False

    def can_run(self):
        return bool(self._env._mask_bits() >> self.index & 1)

    def run(self):
        r = self._env._run(self.index)[1]
        self.done = r is not None or self.done
        return r

    def __repr__(self):
        return "<%s (GPU)>" % self.name


class _GlobalMT:
    """The global ``random``'s MT19937 state read and written in place.

    ``random.getstate()`` + packing and unpacking + ``random.setstate`` cost ~50 us per call
    (a 625-int tuple each way); the drop-in exchanges the state every call.  CPython 3's
    ``_random.Random`` object is ``{PyObject_HEAD; int index; uint32_t state[624];}``
    (Modules/_randommodule.c), so two ``memmove`` of 2.5 KB do the same job, and
    ``gauss_next`` is the Python-level attribute ``random.Random`` keeps.  Enabled only after
    the layout is checked against ``random.getstate()`` (type sizes and the words, both
    directions); otherwise ``ok`` is False and the tuple path runs."""

    def __init__(self):
        self.ok = False
        try:
            self.ok = self._check()
        except Exception:
            self.ok = False

    def _check(self):
        inst = random._inst
        base_t = type(inst).__mro__[-2]  # _random.Random, the C base
        head = object.__basicsize__
        if base_t.__basicsize__ < head + 4 + 4 * 624:
            return False
        self._inst = inst
        self._index = head
        self._state = head + 4
        probe = random.getstate()
        try:
            random.random()  # a state whose index is not 0 or 624
            st = random.getstate()
            ps = _lib.PyState()
            self.load(ps)
            if list(ps.mt) + [ps.index] != list(st[1]):
                return False
            ps.mt[0] ^= 1  # round trip: a store must be what setstate would give
            self.store(ps)
            if random.getstate()[1] != tuple(list(ps.mt) + [ps.index]):
                return False
        finally:
            random.setstate(probe)
        return True

    def load(self, ps):
        base = id(self._inst)
        ctypes.memmove(ctypes.addressof(ps.mt), base + self._state, 4 * 624)
        ps.index = ctypes.c_int.from_address(base + self._index).value
        g = self._inst.gauss_next
        ps.has_gauss = g is not None
        ps.gauss_next = 0.0 if g is None else g

    def store(self, ps):
        base = id(self._inst)
        ctypes.memmove(base + self._state, ctypes.addressof(ps.mt), 4 * 624)
        ctypes.c_int.from_address(base + self._index).value = ps.index
        self._inst.gauss_next = ps.gauss_next if ps.has_gauss else None


_GLOBAL_MT = _GlobalMT()


class TreasureGame:
    """Drop-in for the reference ``TreasureGame`` (treasure_game.py:54-114), one env on the GPU.

    Same surface and Python types: ``reset() -> list[9]``, ``step(a) -> (list[9], int | None,
    bool, {})``, ``available_mask`` (np int array [9]), ``action_space`` Discrete(9),
    ``observation_space`` Box(0, 1, (9,), float32), ``option_names``.

    Random numbers, as in the reference, come by default from Python's process-global
    ``random`` (IM/:2, OB/:9 draw from the module-level ``random``): the constructor's build,
    ``reset`` and ``step`` (and ``option.run``) each read ``random.getstate()``, draw on the
    device (tg_step1_py / tg_reset1_py: one launch, one synchronisation) and store the advanced
    state back with ``random.setstate``, so ``random.seed(s); env = TreasureGame()`` replays
    the reference env draw for draw, and user code that takes its own ``random`` draws in
    between (any of them: random(), randrange, gauss, ...) sees and shapes the same shared
    stream as with the reference.  ``TreasureGame(seed=s)`` instead gives the env a private
    stream equal to ``random.seed(s); TreasureGame()`` in a fresh reference process, and leaves
    the global ``random`` untouched (``share_global_random=False`` with ``seed=None`` draws
    that seed from the global stream).
    ``render(mode='rgb_array')`` returns the frame as a uint8 numpy array [624, 672, 3]
    (TG/:98-105; the sprites are the installed reference's unless ``sprites=`` is given);
    ``mode='human'`` needs gym's image viewer and raises.
    """

    metadata = {"render.modes": ["human", "rgb_array"]}

    def __init__(self, seed=None, device=None, level_dir=None, sprites=None,
                 share_global_random=None):
        self._sprites = sprites
        if share_global_random is None:
            share_global_random = seed is None
        self._shared = bool(share_global_random)
        if self._shared and seed is not None:
            raise ValueError("share_global_random draws from the global random: no seed")
        if seed is None:
            seed = 0 if self._shared else random.getrandbits(64)
        seed = abs(int(seed))  # random.seed(s) keys on abs(s) (CPython random_seed)
        if seed >= 2**64:
            raise ValueError("seed must satisfy |seed| < 2**64 (a two-word init_by_array key)")
        self._vec = TreasureGameVec(1, seed=seed, device=device, level_dir=level_dir)
        self.option_list = [GpuOption(self, k) for k in range(_lib.NUM_ACTIONS)]
        self.option_names = list(OPTION_NAMES)
        self.action_space = Discrete(_lib.NUM_ACTIONS)
        self.observation_space = Box(np.float32(0.0), np.float32(1.0), shape=(_lib.OBS_DIM,))
        self.viewer = None
        self._h_obs = np.zeros(_lib.OBS_DIM, np.float64)  # tg_step1's host outputs
        self._h_rew, self._h_valid, self._h_done = ctypes.c_int32(), ctypes.c_uint8(), ctypes.c_uint8()
        # the step call's arguments, made once: a step is one C call and nothing else.  Its
        # stream is the null stream: every TreasureGame call returns host data, so none of this
        # env's device work is pending when a step starts.
        self._h_mask = ctypes.c_uint16()
        self._p_mask = ctypes.byref(self._h_mask)
        self._step_args = (self._h_obs.ctypes.data, ctypes.byref(self._h_rew),
                           ctypes.byref(self._h_valid), ctypes.byref(self._h_done), None)
        # the shared stream's step works in place on the global random.Random's own words and
        # index (tg_step1_pywords; _GlobalMT checked the layout): no getstate / setstate
        self._pywords = None
        if share_global_random and _GLOBAL_MT.ok:
            base = id(_GLOBAL_MT._inst)
            self._pywords = (base + _GLOBAL_MT._state, base + _GLOBAL_MT._index)
        if self._shared:
            self._py = _lib.PyState()
            # _TreasureGameImpl.__init__'s build draws from the global stream (IM/:31-53)
            self._reset_py(self._h_obs)

    # -- the reference's shared module-level random stream (default) -----------------------------
    _WORDS = struct.Struct("625I")  # tg_pystate's mt[624] + index

    def _load_global(self):
        if _GLOBAL_MT.ok:
            _GLOBAL_MT.load(self._py)
            return None
        st = random.getstate()
        self._WORDS.pack_into(self._py, 0, *st[1])
        g = st[2]
        self._py.has_gauss = g is not None
        self._py.gauss_next = 0.0 if g is None else g
        return st

    def _store_global(self):
        if _GLOBAL_MT.ok:
            _GLOBAL_MT.store(self._py)
            return
        random.setstate((3, self._WORDS.unpack_from(self._py, 0),
                         self._py.gauss_next if self._py.has_gauss else None))

    def _reset_py(self, obs):
        st = self._load_global()
        if st is None:  # in-place load: the replay's start state from the words just loaded
            st = (3, self._WORDS.unpack_from(self._py, 0),
                  self._py.gauss_next if self._py.has_gauss else None)
        check(self._vec._L.tg_reset1_py(self._vec.handle, ctypes.byref(self._py),
                                        obs.ctypes.data, self._vec._stream()), "tg_reset1_py")
        # The reset's draws (IM/:55-73): two uniform(), then gauss twice.  Their stream position
        # is the device's; gauss_next, the cached half of a gauss pair, is left in the global
        # state where user code can read it, so it must be CPython's own sin(x2pi) * g2rad
        # (glibc), not the device's (OCML; they may differ in the last ulp): the same calls are
        # replayed on a private Random from the state the reset started from.
        r = random.Random()
        r.setstate(st)
        r.random()
        r.random()
        r.gauss(0.0, 1.0)
        r.gauss(0.0, 1.0)
        out = r.getstate()
        if out[1] != self._WORDS.unpack_from(self._py, 0):
            raise TgError("tg_reset1_py: the device's stream position differs from CPython's")
        random.setstate(out)

    def reset(self):
        if self._shared:
            self._reset_py(self._h_obs)
            return self._h_obs.tolist()
        # tg_reset1: through the resident server (a reset between episodes does not stop it)
        v = self._vec
        check(v._L.tg_reset1(v.handle, self._h_obs.ctypes.data, None), "tg_reset1")
        return self._h_obs.tolist()

    def _mask_bits(self):
        # tg_available_mask1: through the resident server (a mask read between steps does not
        # stop it); the null stream, as the step
        v = self._vec
        rc = v._L.tg_available_mask1(v.handle, self._p_mask, None)
        if rc:
            check(rc, "tg_available_mask1")
        return int(self._h_mask.value) & 0x1FF

    @property
    def available_mask(self):
        m = self._mask_bits()
        return np.array([(m >> k) & 1 for k in range(_lib.NUM_ACTIONS)])

    def _run(self, a):
        """option_list[a].run() on the device + get_state + done (TG/:91-96): tg_step1 (or
        tg_step1_py over the global stream), one launch whose kernel writes the row into
        pinned host memory, one synchronisation"""
        v = self._vec
        if self._pywords is not None and random._inst is _GLOBAL_MT._inst:
            rc = v._L.tg_step1_pywords(v.handle, a, *self._pywords, *self._step_args)
            if rc:
                check(rc, "tg_step1_pywords")
        elif self._shared:
            self._load_global()
            check(v._L.tg_step1_py(v.handle, a, ctypes.byref(self._py), *self._step_args),
                  "tg_step1_py")
            self._store_global()
        else:
            rc = v._L.tg_step1(v.handle, a, *self._step_args)
            if rc:
                check(rc, "tg_step1")
        r = int(self._h_rew.value) if self._h_valid.value else None
        return self._h_obs.tolist(), r, bool(self._h_done.value)

    def step(self, action):
        a = operator.index(action)  # list indexing accepts ints only (TG/:92)
        if not -_lib.NUM_ACTIONS <= a < _lib.NUM_ACTIONS:
            raise IndexError("list index out of range")
        state, r, done = self._run(a)
        return state, r, done, {}

    def render(self, mode="human", scale=1, gray=False, view=None):
        if mode != "rgb_array":
            raise NotImplementedError("render(mode=%r): only 'rgb_array' (no display / gym "
                                      "image viewer here, TG/:106-110)" % (mode,))
        if getattr(self._vec, "frame_shape", None) is None:
            self._vec.render_init(self._sprites)
        return self._vec.render(scale=scale, gray=gray, view=view).cpu().numpy()[0]

    def close(self):
        if self.viewer is not None:
            self.viewer = None
        self._vec.close()


class ObservationWrapper:
    """The reference's ``ObservationWrapper`` (treasure_game.py:38-51): reset / step return the
    rendered screen instead of the state vector, and step's info carries the state as
    ``info['world_state']``.

    Over a ``TreasureGame`` the screen is a uint8 numpy array [624, 672, 3], as in the
    reference.  Over a ``TreasureGameVec`` it is the batch's frames, a uint8 device tensor
    [N, 624, 672, 3] rendered by one kernel launch into a buffer the wrapper owns
    (overwritten each call), and step returns ``(frames, reward, valid, done, info)``.

    ``scale`` (a divisor of 48) and ``gray`` select the downscaled / grayscale frame of
    ``TreasureGameVec.render``: [N, 78, 84, 1] at ``scale=8, gray=True`` on the default level
    (an extension: the reference's wrapper renders full size only).  ``view=r`` selects the
    agent-centred window of ``TreasureGameVec.render(view=r)`` at that scale and channel count:
    [N, 18, 18, 1] at ``scale=8, gray=True, view=1``.
    """

    def __init__(self, env, sprites=None, scale=1, gray=False, view=None):
        self.env = env
        self._scale, self._gray = int(scale), bool(gray)
        self._view = None if view is None else int(view)
        self._vec = isinstance(env, TreasureGameVec)
        if self._vec:
            env.render_init(sprites)
            if self._view is not None:
                shape = env.frame_shape_view(self._view, self._scale, self._gray)
            else:
                shape = (env.frame_shape if self._scale == 1 and not self._gray
                         else env.frame_shape_scaled(self._scale, self._gray))
            self._frames = torch.empty((env.num_envs,) + shape, dtype=torch.uint8,
                                       device=env.device)
        else:
            if sprites is not None:
                env._sprites = sprites
            # every step renders, and a render (a full-GPU kernel) stops the resident N = 1
            # server: one launch per step costs less than a server stop + relaunch per step
            env._vec.set_serve(False)
        self.action_space = env.action_space
        self.observation_space = env.observation_space

    def __getattr__(self, name):
        return getattr(self.env, name)

    def _screen(self):
        if self._vec:
            return self.env.render(out=self._frames, scale=self._scale, gray=self._gray,
                                   view=self._view)
        return self.env.render(mode="rgb_array", scale=self._scale, gray=self._gray,
                               view=self._view)

    def reset(self, **kwargs):
        self.env.reset(**kwargs)
        return self._screen()

    def step(self, action):
        out = self.env.step(action)
        info = out[-1]
        info["world_state"] = out[0]
        return (self._screen(),) + tuple(out[1:])


class TreasureGameVectorEnv:
    """Gymnasium-style vector env over one ``TreasureGameVec``: the batch steps
    on the device and every output is a device tensor.

    ``reset(seed=None) -> (obs f64 [N, 9], info)``; ``step(actions) -> (obs, reward f32 [N],
    terminated bool [N], truncated bool [N], info)``.  Auto-reset is same-step
    (``metadata["autoreset_mode"] == "SameStep"``): an env that terminates (TG/:95: gold held
    and back in row 0) or is truncated is reset inside the same call, ``obs`` holds its new
    episode's first observation and ``info["final_obs"]`` the last one of the finished
    episode (== ``obs`` for the others).  The reference's ``None`` reward (option could not run,
    OP/:22-23) is reward 0 with ``info["valid"] == 0``.  ``truncated`` is set only when
    ``max_episode_steps`` is given (the reference registers no TimeLimit); those envs are reset
    by a masked ``tg_reset`` on the device, with no host synchronisation.  With
    ``device_time_limit=True`` the limit is the batch's own (``TreasureGameVec``'s
    ``max_episode_steps``): the step's kernels truncate and reset, ``terminated`` / ``truncated``
    are the done row's two bits, and ``episodes(truncated=True)`` lists truncated episodes too.
    The step outputs are the same either way.
    Env g of ``reset(seed=s)`` is ``random.seed(s + g); TreasureGame()`` (contract of
    TreasureGameVec)."""

    metadata = {"autoreset_mode": "SameStep", "render_modes": ["rgb_array"]}

    def __init__(self, num_envs, seed=0, device=None, max_episode_steps=None, level_dir=None,
                 mode="compact", device_time_limit=False):
        self.num_envs = int(num_envs)
        self._kw = dict(device=device, level_dir=level_dir, mode=mode)
        self.max_episode_steps = None if max_episode_steps is None else int(max_episode_steps)
        self.device_time_limit = bool(device_time_limit) and self.max_episode_steps is not None
        if self.device_time_limit:
            self._kw["max_episode_steps"] = self.max_episode_steps
        self.single_action_space = Discrete(_lib.NUM_ACTIONS)
        self.single_observation_space = Box(np.float32(0.0), np.float32(1.0),
                                            shape=(_lib.OBS_DIM,))
        self.action_space = MultiDiscrete([_lib.NUM_ACTIONS] * self.num_envs)
        self.observation_space = Box(np.float32(0.0), np.float32(1.0),
                                     shape=(self.num_envs, _lib.OBS_DIM))
        self._make(seed)

    def _make(self, seed):
        old = getattr(self, "env", None)
        if old is not None:
            old.close()
        # copy=True: every returned tensor is the caller's own (gymnasium loops keep obs across
        # steps: obs_t must not change when the next step writes the library's buffers)
        self.env = TreasureGameVec(self.num_envs, seed=seed, autoreset=True, copy=True, **self._kw)
        self.device = self.env.device
        self._len = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)

    def reset(self, seed=None, options=None):
        if seed is not None:
            self._make(int(seed))
        obs = self.env.reset()
        self._len.zero_()
        return obs, {}

    def step(self, actions):
        obs, rew, valid, done, info = self.env.step(actions)
        final = info["final_obs"]
        if self.device_time_limit:
            return (obs, rew.to(torch.float32), (done & DONE_TERMINATED).bool(),
                    (done & DONE_TRUNCATED).bool(), {"final_obs": final, "valid": valid})
        terminated = done.bool()
        self._len += 1
        self._len.masked_fill_(terminated, 0)
        if self.max_episode_steps is not None:
            truncated = self._len >= self.max_episode_steps
            self._len.masked_fill_(truncated, 0)
            obs = self.env.reset(truncated.to(torch.uint8))  # masked reset, obs of every env
        else:
            truncated = torch.zeros_like(terminated)
        return obs, rew.to(torch.float32), terminated, truncated, {"final_obs": final,
                                                                   "valid": valid}

    def available_mask(self):
        return self.env.available_mask()

    def episodes(self, cap=None, truncated=False):
        """(env, return, length) of the terminated episodes (device queue, TreasureGameVec);
        with ``device_time_limit`` the truncated ones too (``truncated=True`` marks them)"""
        return self.env.episodes(cap, truncated)

    def close(self):
        self.env.close()


def make_vec(id="treasure_game-v0", num_envs=1, **kwargs):
    """gymnasium.make_vec stand-in: a TreasureGameVectorEnv of ``num_envs`` envs."""
    if id != "treasure_game-v0":
        raise KeyError("unknown env id %r" % (id,))
    return TreasureGameVectorEnv(num_envs, **kwargs)
