"""Thin torch-tensor wrappers over the C-ABI (one function per exported kernel group).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every bit of
arithmetic on the hot path is a hand-written HIP kernel in deeprl_amd/csrc reached through
deeprl_amd._lib.  All tensors must be CUDA(ROCm) tensors; there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from ._lib import DraError, lib, ptr, ptr_array, stream_ptr

ACT = {None: 0, "none": 0, "relu": 1, "tanh": 2}
_f32 = torch.float32


def _dev(t):
    if not t.is_cuda:
        raise DraError("deeprl_amd ops need device tensors (got %s); there is no CPU fallback" % t.device)
    return t


def _c(t, dtype=None):
    _dev(t)
    if dtype is not None and t.dtype != dtype:
        raise DraError("expected dtype %s, got %s" % (dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------ ring
class Ring:
    """HBM ring handle (dra_ring_*).  Host bookkeeping (pos/size) lives in component/replay.py."""

    def __init__(self, capacity, frame_bytes, action_bytes, history, n_step, discount):
        h = ctypes.c_void_p()
        lib.dra_ring_create(ctypes.byref(h), int(capacity), int(frame_bytes), int(action_bytes), int(history),
                            int(n_step), float(discount))
        self.h = h
        self.capacity, self.frame_bytes, self.action_bytes = int(capacity), int(frame_bytes), int(action_bytes)
        self.history, self.n_step = int(history), int(n_step)

    def arrays(self):
        """(frames u8[capacity * frame_bytes], actions u8[capacity * action_bytes], rewards f64[capacity], masks i32[capacity])
        as tensors over the ring's own device memory (true resume dumps / restores them)."""
        f, a, r, m = self.pointers()
        return (_wrap_device_pointer(f, self.capacity * self.frame_bytes, torch.uint8),
                _wrap_device_pointer(a, self.capacity * self.action_bytes, torch.uint8),
                _wrap_device_pointer(r, self.capacity, torch.float64), _wrap_device_pointer(m, self.capacity, torch.int32))

    def close(self):
        if self.h:
            lib.dra_ring_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def put_host(self, slot, frame, action, reward, mask):
        frame = np.ascontiguousarray(frame)
        action = np.ascontiguousarray(action)
        if frame.nbytes != self.frame_bytes or action.nbytes != self.action_bytes:
            raise DraError("put_host: frame/action byte size mismatch (%d/%d vs %d/%d)" %
                           (frame.nbytes, action.nbytes, self.frame_bytes, self.action_bytes))
        lib.dra_ring_put_host(self.h, int(slot), frame.ctypes.data_as(ctypes.c_void_p),
                              action.ctypes.data_as(ctypes.c_void_p), float(reward), int(mask), stream_ptr())

    def put_device(self, slot0, frames, actions=None, rewards=None, masks=None, action_val=0, reward_val=0.0,
                   mask_val=1, count=1):
        lib.dra_ring_put(self.h, int(slot0), int(count), ptr(_c(frames)), ptr(actions), int(action_val), ptr(rewards),
                         float(reward_val), ptr(masks), int(mask_val), stream_ptr())

    def put_rows(self, count, frames, frame_stride, actions, rewards, masks, slot0_dev=None, slot0=0):
        """The `count` <= 8 transitions of one agent step (dra_ring_put_rows): first slot from the device word slot0_dev (int64
        tensor) or by value, wrapping at the capacity; frame k starts frame_stride bytes behind frame k - 1 of `frames`."""
        if actions.dtype != torch.int64 or rewards.dtype != torch.float64 or masks.dtype != torch.int32 or \
                (slot0_dev is not None and slot0_dev.dtype != torch.int64):
            raise DraError("put_rows: actions int64, rewards float64, masks int32, slot0_dev int64")
        if min(actions.numel(), rewards.numel(), masks.numel()) < count:
            raise DraError("put_rows: %d transitions need %d actions / rewards / masks" % (count, count))
        lib.dra_ring_put_rows(self.h, ptr(slot0_dev), int(slot0), int(count), ptr(_dev(frames)), int(frame_stride), ptr(_dev(actions)),
                              ptr(_dev(rewards)), ptr(_dev(masks)), stream_ptr())

    def fill_synthetic(self, slot0, count, counter0, seed, n_actions=4, done_period=800):
        lib.dra_ring_fill_synthetic(self.h, int(slot0), int(count), int(counter0), int(seed), int(n_actions),
                                    int(done_period), stream_ptr())

    def gather(self, idx, state_shape, state_dtype, action_dtype=torch.int64, want_f32=False, out=None, block=True):
        """idx: int64 device tensor [B].  Returns dict of device tensors shaped like the reference's sample().  block (and no
        caller-owned `out`): state / next_state are two VIEWS of one [B, history + n_step, ...] block in which every frame of a
        sample's run is written once (dra_ring_gather_block) -- same values, non-contiguous along the batch axis."""
        idx = _c(idx, torch.int64)
        b = idx.numel()
        dev = idx.device
        if out is not None and out.get("block") is not None:        # a dict this method returned in block form: refill in place
            lib.dra_ring_gather_block(self.h, ptr(idx), b, ptr(out["block"]), ptr(out["action"]), ptr(out["reward"]), ptr(out["mask"]),
                                      ptr(out.get("reward_f32")), ptr(out.get("mask_f32")), stream_ptr())
            return out
        if out is None and block:
            h, n = self.history, self.n_step
            blk = torch.empty((b, h + n) + tuple(state_shape), dtype=state_dtype, device=dev)
            esize = torch.empty(0, dtype=action_dtype).element_size()
            ashape = (b,) if self.action_bytes == esize else (b, self.action_bytes // esize)
            out = dict(block=blk, state=blk[:, :h] if h > 1 else blk[:, 0], next_state=blk[:, n:] if h > 1 else blk[:, n],
                       action=torch.empty(ashape, dtype=action_dtype, device=dev),
                       reward=torch.empty(b, dtype=torch.float64, device=dev), mask=torch.empty(b, dtype=torch.int32, device=dev))
            if want_f32:
                out["reward_f32"] = torch.empty(b, dtype=_f32, device=dev)
                out["mask_f32"] = torch.empty(b, dtype=_f32, device=dev)
            lib.dra_ring_gather_block(self.h, ptr(idx), b, ptr(blk), ptr(out["action"]), ptr(out["reward"]), ptr(out["mask"]),
                                      ptr(out.get("reward_f32")), ptr(out.get("mask_f32")), stream_ptr())
            return out
        if out is None:
            stack = (b, self.history) + tuple(state_shape) if self.history > 1 else (b,) + tuple(state_shape)
            esize = torch.empty(0, dtype=action_dtype).element_size()
            ashape = (b,) if self.action_bytes == esize else (b, self.action_bytes // esize)
            out = dict(state=torch.empty(stack, dtype=state_dtype, device=dev),
                       next_state=torch.empty(stack, dtype=state_dtype, device=dev),
                       action=torch.empty(ashape, dtype=action_dtype, device=dev),
                       reward=torch.empty(b, dtype=torch.float64, device=dev),
                       mask=torch.empty(b, dtype=torch.int32, device=dev))
            if want_f32:
                out["reward_f32"] = torch.empty(b, dtype=_f32, device=dev)
                out["mask_f32"] = torch.empty(b, dtype=_f32, device=dev)
        lib.dra_ring_gather(self.h, ptr(idx), b, ptr(out["state"]), ptr(out["next_state"]), ptr(out["action"]),
                            ptr(out["reward"]), ptr(out["mask"]), ptr(out.get("reward_f32")), ptr(out.get("mask_f32")),
                            stream_ptr())
        return out

    def pointers(self):
        ps = [ctypes.c_void_p() for _ in range(4)]
        lib.dra_ring_pointers(self.h, *[ctypes.byref(p) for p in ps])
        return [p.value for p in ps]


def u8_to_f32(x_u8, lut):
    _dev(x_u8)
    if x_u8.dtype != torch.uint8:
        raise DraError("expected dtype %s, got %s" % (torch.uint8, x_u8.dtype))
    out = torch.empty(x_u8.shape, dtype=_f32, device=x_u8.device)
    if (not x_u8.is_contiguous() and x_u8.dim() >= 2 and x_u8.shape[0] > 0 and x_u8[0].is_contiguous()
            and x_u8[0].numel() % 16 == 0 and x_u8.stride(0) % 16 == 0 and x_u8.stride(0) >= x_u8[0].numel()
            and x_u8.data_ptr() % 16 == 0):
        # rows that are contiguous inside and a fixed distance apart (the state / next_state views of Ring.gather): read in place
        lib.dra_u8_to_f32_lut_rows(ptr(x_u8), ptr(out), int(x_u8.shape[0]), int(x_u8[0].numel()), int(x_u8.stride(0)),
                                   ptr(_c(lut, _f32)), stream_ptr())
        return out
    x = x_u8 if x_u8.is_contiguous() else x_u8.contiguous()
    lib.dra_u8_to_f32_lut(ptr(x), ptr(out), x.numel(), ptr(_c(lut, _f32)), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------ sum tree
class SumTree:
    def __init__(self, capacity):
        h = ctypes.c_void_p()
        lib.dra_sumtree_create(ctypes.byref(h), int(capacity))
        self.h = h
        self.capacity = int(capacity)
        self.n_nodes = 2 * self.capacity - 1

    def close(self):
        if self.h:
            lib.dra_sumtree_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, leaf_idx, prio, ordered=False):
        leaf_idx, prio = _c(leaf_idx, torch.int64), _c(prio, torch.float64)
        lib.dra_sumtree_update(self.h, ptr(leaf_idx), ptr(prio), leaf_idx.numel(), int(bool(ordered)), stream_ptr())

    def set(self, leaf_idx, prio):
        lib.dra_sumtree_set(self.h, int(leaf_idx), float(prio), stream_ptr())

    def set_from(self, leaf_idx, prio_dev):
        """set() with the priority read from device memory (f64 tensor, first element)."""
        lib.dra_sumtree_set_from(self.h, int(leaf_idx), ptr(prio_dev), stream_ptr())

    def set_many_from(self, write0, n, prio_dev, stat=None, stream=None):
        """n consecutive adds at write cursor write0.. (mod capacity), all at the device-resident priority prio_dev[0].  stat:
        commit_f32's f64[2] {running max, running min}; inside its exactness bound the adds run level-parallel, outside it (or
        without a stat) as the reference's delta walks one after another."""
        lib.dra_sumtree_set_many_from(self.h, int(write0), int(n), ptr(prio_dev), ptr(stat), stream_ptr(stream))

    def sample_into(self, u, out_idx, out_p, out_total, stream=None):
        """sample() into caller-provided buffers (e.g. pinned host memory the kernel writes directly; `u` may be pinned too)."""
        lib.dra_sumtree_sample(self.h, ptr(u), u.numel(), ptr(out_idx), ptr(out_p), ptr(out_total), stream_ptr(stream))

    def commit_f32(self, leaf_idx, pos, prio_f32, stat, force_ordered=False, stream=None):
        """Priority write-back with the values still on the device: leaf_idx[i] <- f64(prio_f32[pos[i]]); stat (f64[2] device
        tensor) = {running max, running min} over ALL of prio_f32 (dra_sumtree_commit_f32)."""
        n = 0 if leaf_idx is None else leaf_idx.numel()
        lib.dra_sumtree_commit_f32(self.h, ptr(leaf_idx) if n else None, ptr(pos) if n else None, n, ptr(prio_f32),
                                   prio_f32.numel(), ptr(stat), int(bool(force_ordered)), stream_ptr(stream))

    def sample(self, u):
        u = _c(u, torch.float64)
        b = u.numel()
        idx = torch.empty(b, dtype=torch.int64, device=u.device)
        p = torch.empty(b, dtype=torch.float64, device=u.device)
        total = torch.empty(1, dtype=torch.float64, device=u.device)
        lib.dra_sumtree_sample(self.h, ptr(u), b, ptr(idx), ptr(p), ptr(total), stream_ptr())
        return idx, p, total

    def rebuild(self):
        lib.dra_sumtree_rebuild(self.h, stream_ptr())

    def as_tensor(self):
        """Zero-copy f64 view of the heap array (for tests / checkpoints)."""
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        lib.dra_sumtree_pointer(self.h, ctypes.byref(p), ctypes.byref(n))
        return _wrap_device_pointer(p.value, n.value, torch.float64)


def _wrap_device_pointer(addr, numel, dtype):
    """torch view over library-owned HBM via __cuda_array_interface__ (no copy)."""
    typestr = {torch.float64: "<f8", torch.float32: "<f4", torch.uint8: "|u1", torch.int64: "<i8",
               torch.int32: "<i4"}[dtype]

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = dict(shape=(int(numel),), typestr=typestr, data=(int(addr), False), version=2)
    return torch.as_tensor(h, device="cuda")


# ------------------------------------------------------------------------------------------ losses
def _action_args(action):
    if action.dtype == torch.int64:
        return ptr(_c(action)), 1
    if action.dtype == _f32:
        return ptr(_c(action)), 0
    raise DraError("action must be int64 or float32, got %s" % action.dtype)


def td_loss(q, q_next_target, action, reward, mask, gamma_n, q_next_online=None, sampling_prob=None, beta=0.0,
            replay_eps=0.01, replay_alpha=0.5):
    q, qt = _c(q, _f32), _c(q_next_target, _f32)
    b, a = q.shape
    dev = q.device
    out = dict(loss=torch.empty((), dtype=_f32, device=dev), dq=torch.empty_like(q),
               delta=torch.empty(b, dtype=_f32, device=dev))
    if sampling_prob is not None:
        out["prio"] = torch.empty(b, dtype=_f32, device=dev)
        out["weights"] = torch.empty(b, dtype=_f32, device=dev)
    ap, ai = _action_args(action)
    lib.dra_td_loss(ptr(q), ptr(qt), ptr(None if q_next_online is None else _c(q_next_online, _f32)), ap, ai,
                    ptr(_c(reward, _f32)), ptr(_c(mask, _f32)), b, a, float(gamma_n),
                    ptr(None if sampling_prob is None else _c(sampling_prob, _f32)), float(beta), float(replay_eps),
                    float(replay_alpha), ptr(out["loss"]), ptr(out["dq"]), ptr(out["delta"]), ptr(out.get("prio")),
                    ptr(out.get("weights")), stream_ptr())
    return out


def c51_loss(logits, logits_next_target, action, reward, mask, gamma_n, atoms, v_min, v_max,
             logits_next_online=None, weights=None):
    lg, lt = _c(logits, _f32), _c(logits_next_target, _f32)
    b, a, n = lg.shape
    out = dict(kl=torch.empty(b, dtype=_f32, device=lg.device), dlogits=torch.empty_like(lg))
    ap, ai = _action_args(action)
    lib.dra_c51_loss(ptr(lg), ptr(lt), ptr(None if logits_next_online is None else _c(logits_next_online, _f32)), ap,
                     ai, ptr(_c(reward, _f32)), ptr(_c(mask, _f32)), b, a, n, float(gamma_n), float(v_min),
                     float(v_max), ptr(_c(atoms, _f32)), ptr(out["kl"]), ptr(out["dlogits"]),
                     ptr(None if weights is None else _c(weights, _f32)), stream_ptr())
    out["loss"] = weighted_mean(out["kl"], weights)
    return out


def qr_loss(theta, theta_next_target, action, reward, mask, gamma_n):
    th, tt = _c(theta, _f32), _c(theta_next_target, _f32)
    b, a, n = th.shape
    dev = th.device
    ws = torch.empty(b * n, dtype=_f32, device=dev)
    out = dict(loss_vec=torch.empty(n, dtype=_f32, device=dev), loss=torch.empty((), dtype=_f32, device=dev),
               dtheta=torch.empty_like(th))
    ap, ai = _action_args(action)
    lib.dra_qr_loss(ptr(th), ptr(tt), ap, ai, ptr(_c(reward, _f32)), ptr(_c(mask, _f32)), b, a, n, float(gamma_n),
                    ptr(ws), ptr(out["loss_vec"]), ptr(out["loss"]), ptr(out["dtheta"]), stream_ptr())
    return out


def per_weights(loss_vec, sampling_prob, beta, replay_eps, replay_alpha):
    sp = _c(sampling_prob, _f32)
    b = sp.numel()
    prio = torch.empty(b, dtype=_f32, device=sp.device) if loss_vec is not None else None
    w = torch.empty(b, dtype=_f32, device=sp.device)
    lib.dra_per_weights(ptr(None if loss_vec is None else _c(loss_vec, _f32)), ptr(sp), b, float(beta),
                        float(replay_eps), float(replay_alpha), ptr(prio), ptr(w), stream_ptr())
    return prio, w


def weighted_mean(x, w=None):
    x = _c(x, _f32)
    out = torch.empty((), dtype=_f32, device=x.device)
    lib.dra_weighted_mean(ptr(x), ptr(None if w is None else _c(w, _f32)), x.numel(), ptr(out), stream_ptr())
    return out


def ppo_loss(log_pi_a, entropy, v, old_log_pi_a, adv, ret, ratio_clip, entropy_weight):
    lp = _c(log_pi_a, _f32)
    m = lp.numel()
    out3 = torch.empty(3, dtype=_f32, device=lp.device)
    g = [torch.empty(lp.shape, dtype=_f32, device=lp.device) for _ in range(3)]
    lib.dra_ppo_loss(ptr(lp), ptr(_c(entropy, _f32)), ptr(_c(v, _f32)), ptr(_c(old_log_pi_a, _f32)), ptr(_c(adv, _f32)),
                     ptr(_c(ret, _f32)), m, float(ratio_clip), float(entropy_weight), ptr(out3), ptr(g[0]), ptr(g[1]),
                     ptr(g[2]), stream_ptr())
    return out3, g


def a2c_loss(log_pi_a, entropy, v, adv, ret, entropy_weight, value_loss_weight):
    lp = _c(log_pi_a, _f32)
    m = lp.numel()
    out4 = torch.empty(4, dtype=_f32, device=lp.device)
    g = [torch.empty(lp.shape, dtype=_f32, device=lp.device) for _ in range(3)]
    lib.dra_a2c_loss(ptr(lp), ptr(_c(entropy, _f32)), ptr(_c(v, _f32)), ptr(_c(adv, _f32)), ptr(_c(ret, _f32)), m,
                     float(entropy_weight), float(value_loss_weight), ptr(out4), ptr(g[0]), ptr(g[1]), ptr(g[2]),
                     stream_ptr())
    return out4, g


def _gauss_head_args(z, std, action):
    z, std, action = _c(z, _f32), _c(std, _f32), _c(action, _f32)
    if z.dim() != 2 or tuple(action.shape) != tuple(z.shape) or std.numel() != z.shape[1] or z.shape[0] < 1:
        raise DraError("gauss_head: z / action [n, A] and std [A] expected, got %s, %s, %s" %
                       (tuple(z.shape), tuple(action.shape), tuple(std.shape)))
    return z, std, action


def gauss_head_fwd(z, std, action):
    """network_heads.py:200-214 behind fc_action for given actions (csrc/a2c_mlp.hip): z [n, A] = fc_action's output, std [A],
    action [n, A] -> (mean = tanh(z) [n, A], log_pi_a [n, 1], entropy [n, 1]) with scale = softplus(std)."""
    z, std, action = _gauss_head_args(z, std, action)
    n, a_dim = z.shape
    mean = torch.empty_like(z)
    lp = torch.empty((n, 1), dtype=_f32, device=z.device)
    ent = torch.empty((n, 1), dtype=_f32, device=z.device)
    lib.dra_gauss_head_fwd(ptr(z), ptr(std), ptr(action), n, a_dim, ptr(mean), ptr(lp), ptr(ent), stream_ptr())
    return mean, lp, ent


def gauss_head_bwd(z, std, action, g_log_pi_a, g_entropy, dstd=None):
    """Gradient of gauss_head_fwd for g_log_pi_a, g_entropy [n, 1] -> (dz [n, A], dstd [A]); `dstd`: a contiguous f32 [A]
    tensor to write into (a parameter's .grad slot).  The reduction over n has a fixed order: equal bits on every launch."""
    z, std, action = _gauss_head_args(z, std, action)
    n, a_dim = z.shape
    g_lp, g_ent = _c(g_log_pi_a, _f32), _c(g_entropy, _f32)
    if g_lp.numel() != n or g_ent.numel() != n:
        raise DraError("gauss_head_bwd: one gradient per row expected")
    dz = torch.empty_like(z)
    if dstd is None:
        dstd = torch.empty(a_dim, dtype=_f32, device=z.device)
    elif not dstd.is_cuda or dstd.dtype != _f32 or not dstd.is_contiguous() or dstd.numel() != a_dim:
        raise DraError("gauss_head_bwd: dstd must be a contiguous f32 device tensor of action_dim elements")
    lib.dra_gauss_head_bwd(ptr(z), ptr(std), ptr(action), ptr(g_lp), ptr(g_ent), n, a_dim, ptr(dz), ptr(dstd), stream_ptr())
    return dz, dstd


# ------------------------------------------------------------------------------------------ scan
def gae(reward, mask, value, gamma, tau, use_gae):
    """reward, mask: [T,N(,1)] f32; value: [T+1,N(,1)] f32 -> (adv, ret) shaped like reward."""
    r, m, v = _c(reward, _f32), _c(mask, _f32), _c(value, _f32)
    t_len = r.shape[0]
    n_env = r.numel() // t_len
    if v.numel() != (t_len + 1) * n_env or m.numel() != r.numel():
        raise DraError("gae: shape mismatch")
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    lib.dra_gae(ptr(r), ptr(m), ptr(v), t_len, n_env, float(gamma), float(tau), int(bool(use_gae)), ptr(adv), ptr(ret),
                stream_ptr())
    return adv, ret


def adv_normalize_(adv):
    a = _dev(adv)
    if not a.is_contiguous() or a.dtype != _f32:
        raise DraError("adv_normalize_ needs a contiguous f32 tensor")
    lib.dra_adv_normalize(ptr(a), a.numel(), stream_ptr())
    return adv


# ------------------------------------------------------------------------------------------ contractions
_CONV_GEOM = {1: (4, 84, 32, 8, 4), 2: (32, 20, 64, 4, 2), 3: (64, 9, 64, 3, 1)}  # C, H, OC, K, S


def conv_layer_for(weight_shape, stride, in_hw):
    """Which NatureConvBody layer (1..3) a Conv2d is, or None."""
    for layer, (c, h, oc, k, s) in _CONV_GEOM.items():
        if tuple(weight_shape) == (oc, c, k, k) and stride == s and in_hw == h:
            return layer
    return None


def conv_out_shape(layer, batch):
    c, h, oc, k, s = _CONV_GEOM[layer]
    o = (h - k) // s + 1
    return (batch, oc, o, o)


def conv_fwd(layer, xs, ws, bs, act="relu", u8_coef=None):
    """Batched forward: lists of nz inputs / weights / biases -> list of nz outputs (one launch)."""
    nz = len(xs)
    c, h, oc, k, s = _CONV_GEOM[layer]
    batch = xs[0].shape[0]
    is_u8 = xs[0].dtype == torch.uint8
    if is_u8 and u8_coef is None:
        raise DraError("uint8 input needs u8_coef")
    xs = [_c(x, torch.uint8 if is_u8 else _f32) for x in xs]
    for x in xs:
        if tuple(x.shape) != (batch, c, h, h):
            raise DraError("conv_fwd layer %d expects [B,%d,%d,%d], got %s" % (layer, c, h, h, tuple(x.shape)))
    ws = [_c(w, _f32) for w in ws]
    bs = [_c(b, _f32) for b in bs]
    ys = [torch.empty(conv_out_shape(layer, batch), dtype=_f32, device=xs[0].device) for _ in range(nz)]
    lib.dra_conv_fwd(layer, nz, ptr_array(xs), ptr_array(ws), ptr_array(bs), ptr_array(ys), batch, int(is_u8),
                     float(u8_coef if is_u8 else 1.0), ACT[act], stream_ptr())
    return ys


def conv_bwd_w(layer, dy, x, ksplit=16, u8_coef=None, slabs=None):
    """Returns (dw_slabs [ksplit, OC*K], db_slabs [ksplit, OC]) views of one slab buffer."""
    c, h, oc, k, s = _CONV_GEOM[layer]
    kk = c * k * k
    batch = x.shape[0]
    is_u8 = x.dtype == torch.uint8
    stride = oc * kk + oc
    stride = (stride + 3) // 4 * 4
    if slabs is None:
        slabs = torch.empty(ksplit * stride, dtype=_f32, device=x.device)
    dw0 = slabs
    lib.dra_conv_bwd_w(layer, ptr(_c(dy, _f32)), ptr(_c(x)), ptr(slabs), ctypes.c_void_p(slabs.data_ptr() + 4 * oc * kk),
                       stride, ksplit, batch, int(is_u8), float(u8_coef if is_u8 else 1.0), stream_ptr())
    v = dw0.view(ksplit, stride)
    return v[:, :oc * kk], v[:, oc * kk:oc * kk + oc]


def to_koc(w):
    """[OC,C,KH,KW] -> the [K=(c,kh,kw)][OC] layout of conv_v2.hip (a torch copy; test / glue helper)."""
    return w.permute(1, 2, 3, 0).contiguous().view(-1, w.shape[0])


def from_koc(wt, shape):
    oc, c, kh, kw = shape
    return wt.view(c, kh, kw, oc).permute(3, 0, 1, 2).contiguous()


def conv_fwd_koc(layer, xs, wts, bs, act="relu", u8_coef=None):
    nz = len(xs)
    c, h, oc, k, s = _CONV_GEOM[layer]
    batch = xs[0].shape[0]
    is_u8 = xs[0].dtype == torch.uint8
    xs = [_c(x, torch.uint8 if is_u8 else _f32) for x in xs]
    wts = [_c(w, _f32) for w in wts]
    bs = [_c(b, _f32) for b in bs]
    ys = [torch.empty(conv_out_shape(layer, batch), dtype=_f32, device=xs[0].device) for _ in range(nz)]
    lib.dra_conv_fwd_koc(layer, nz, ptr_array(xs), ptr_array(wts), ptr_array(bs), ptr_array(ys), batch, int(is_u8),
                         float(u8_coef if is_u8 else 1.0), ACT[act], stream_ptr())
    return ys


def conv_bwd_w_koc(layer, dy, x, ksplit=16, u8_coef=None):
    """Returns (dwt_slabs [ksplit, K*OC] in KOC layout, db_slabs [ksplit, OC])."""
    c, h, oc, k, s = _CONV_GEOM[layer]
    kk = c * k * k
    is_u8 = x.dtype == torch.uint8
    stride = (oc * kk + oc + 3) // 4 * 4
    slabs = torch.empty(ksplit * stride, dtype=_f32, device=x.device)
    lib.dra_conv_bwd_w_koc(layer, ptr(_c(dy, _f32)), ptr(_c(x)), ptr(slabs), ctypes.c_void_p(slabs.data_ptr() + 4 * oc * kk),
                           stride, ksplit, x.shape[0], int(is_u8), float(u8_coef if is_u8 else 1.0), stream_ptr())
    v = slabs.view(ksplit, stride)
    return v[:, :oc * kk], v[:, oc * kk:oc * kk + oc]


def conv_bwd_x_koc(layer, dy, wt, xact=None, act="relu"):
    c, h, oc, k, s = _CONV_GEOM[layer]
    batch = dy.shape[0]
    dx = torch.empty((batch, c, h, h), dtype=_f32, device=dy.device)
    lib.dra_conv_bwd_x_koc(layer, ptr(_c(dy, _f32)), ptr(_c(wt, _f32)), ptr(None if xact is None else _c(xact, _f32)),
                           ptr(dx), batch, ACT[act], stream_ptr())
    return dx


# variant bits of the fused / one-pass kernels (include/deeprl_amd.h DRA_VAR_*)
VAR_FUSED_BWD, VAR_ONESHOT_DGRAD, VAR_ONESHOT_FWD, VAR_ONESHOT_WGRAD = 1, 2, 4, 8
VAR_PINNED_IDX, VAR_ACTOR_V2, VAR_ACTOR_PARAMS, VAR_PIPE_GATHER, VAR_CU_PARTITION, VAR_ACTOR_V3 = 16, 32, 64, 128, 256, 512
VAR_ACTOR_FUSED_HEAD = 1024
VAR_GATHER_IN_GRAPH = 2048
VAR_ACTOR_RING = 4096
VAR_ACTOR_FUSED_CONV1 = 8192
VAR_GATHER_ON_UPDATE = 16384
VAR_RING_DIRECT = 32768
VAR_IDX_PREFETCH = 131072
VAR_DGRAD_SCATTER = 262144    # conv2 / conv3 input gradient at batch >= 256 in scatter (col2im) form
VAR_LATE_FOLD = 524288
VAR_ACTOR_MEGA = 1048576
VAR_DEFER_FC4 = 8388608       # fc4's segment of the optimizer step rides in the next update's forward launches
VAR_ACTOR_PERSIST = 16777216  # the whole agent step of the device actor as one launch ({value, tag} hand-overs)
VAR_FWD_CHAIN = 33554432      # conv1 + conv2 + conv3 of the update's forward as one chained launch
VAR_BWD_CHAIN = 67108864      # conv3 + conv2 + conv1 backward of the update as one chained launch
VAR_FLAG_SYNC = 134217728     # the steady-state pipelined step without events (device counts + pinned words)
VAR_LANE_EAGER = 268435456    # ... and the update as plain launches instead of a graph replay
VAR_TARGET_AHEAD = 536870912  # target(next_states) of update t + 1 issued one call early, under update t (needs the next indices)
VAR_BWD_CHAIN_FC = 1073741824 # fc4's + the head's backward as leading roles of the chained backward launch
VAR_HEAD_CHAIN = 65536        # head launch + fc4's / the head's backward launch as one launch in dependency order
VAR_ALL = 2097151 | 8388608 | 16777216 | 33554432 | 67108864 | 134217728 | 268435456 | 536870912 | 1073741824 | 65536


def set_tuning(mask):
    """Process-wide default variant mask for learners created afterwards (dra_set_tuning)."""
    lib.dra_set_tuning(int(mask))


def get_tuning():
    m = ctypes.c_int(0)
    lib.dra_get_tuning(ctypes.byref(m))
    return m.value


def conv_wgrad_slabs(layer, batch, ksplit, variant):
    n = ctypes.c_int(0)
    lib.dra_conv_wgrad_slabs(int(layer), int(batch), int(ksplit), int(variant), ctypes.byref(n))
    return n.value


def conv_bwd_fused(layer, dy, x, wt=None, xact=None, ksplit=16, u8_coef=None, act="relu", variant=0):
    """One launch: KOC weight / bias gradient slabs (+ the input gradient for layers 2, 3).
    Returns (dwt_slabs [n_slabs, K*OC], db_slabs [n_slabs, OC], dx or None, the flat slab buffer)."""
    c, h, oc, k, s = _CONV_GEOM[layer]
    kk = c * k * k
    batch = x.shape[0]
    is_u8 = x.dtype == torch.uint8
    stride = (oc * kk + oc + 3) // 4 * 4
    n_slabs = conv_wgrad_slabs(layer, batch, ksplit, variant)
    slabs = torch.full((n_slabs * stride,), float("nan"), dtype=_f32, device=x.device)
    dx = torch.full((batch, c, h, h), float("nan"), dtype=_f32, device=x.device) if layer > 1 else None
    lib.dra_conv_bwd_fused(layer, ptr(_c(dy, _f32)), ptr(_c(x)), ptr(None if wt is None else _c(wt, _f32)),
                           ptr(None if xact is None else _c(xact, _f32)), ptr(slabs),
                           ctypes.c_void_p(slabs.data_ptr() + 4 * oc * kk), stride, ksplit, ptr(dx), batch, int(is_u8),
                           float(u8_coef if is_u8 else 1.0), ACT[act], int(variant), stream_ptr())
    v = slabs.view(n_slabs, stride)
    return v[:, :oc * kk], v[:, oc * kk:oc * kk + oc], dx, slabs


def conv_bwd_fused_koc(layer, dy, x, wt, ksplit=16, u8_coef=None, variant=0, xact=None):
    """Production form of conv_bwd_fused (generic autograd path): dy = gradient w.r.t. this layer's pre-activation,
    wt = KOC weights.  One launch -> (dx or None, slab buffer [n_slabs * stride], n_slabs, stride); slab s holds
    dWt [K*OC] then db [OC]; the caller folds them (grad_sqnorm)."""
    c, h, oc, k, s = _CONV_GEOM[layer]
    kk = c * k * k
    batch = x.shape[0]
    is_u8 = x.dtype == torch.uint8
    stride = (oc * kk + oc + 3) // 4 * 4
    n_slabs = conv_wgrad_slabs(layer, batch, ksplit, variant)
    slabs = torch.empty(n_slabs * stride, dtype=_f32, device=x.device)
    if stride != oc * kk + oc:
        slabs.view(n_slabs, stride)[:, oc * kk + oc:].zero_()      # alignment gap is folded too: keep it finite
    dx = torch.empty((batch, c, h, h), dtype=_f32, device=x.device) if layer > 1 else None
    lib.dra_conv_bwd_fused(layer, ptr(_c(dy, _f32)), ptr(_c(x)), ptr(_c(wt, _f32)), ptr(None if xact is None else _c(xact, _f32)),
                           ptr(slabs), ctypes.c_void_p(slabs.data_ptr() + 4 * oc * kk), stride, ksplit, ptr(dx), batch, int(is_u8),
                           float(u8_coef if is_u8 else 1.0), ACT["relu"], int(variant), stream_ptr())
    return dx, slabs, n_slabs, stride


def fc_bwd_fused(dq, h4, dh4, x3, w4, act="relu", variant=0):
    """One launch: head weight gradient, fc4 weight gradient, fc4 input gradient (hidden = 512)."""
    dq, h4, dh4, x3, w4 = [_c(t, _f32) for t in (dq, h4, dh4, x3, w4)]
    batch, a = dq.shape
    fin = x3.shape[1]
    dev = dq.device
    nan = float("nan")
    dwh = torch.full((a, 512), nan, dtype=_f32, device=dev)
    dbh = torch.full((a,), nan, dtype=_f32, device=dev)
    dw4 = torch.full((512, fin), nan, dtype=_f32, device=dev)
    db4 = torch.full((512,), nan, dtype=_f32, device=dev)
    dx3 = torch.full((batch, fin), nan, dtype=_f32, device=dev)
    lib.dra_fc_bwd_fused(ptr(dq), ptr(h4), ptr(dh4), ptr(x3), ptr(w4), ptr(dwh), ptr(dbh), ptr(dw4), ptr(db4), ptr(dx3),
                         batch, a, fin, ACT[act], int(variant), stream_ptr())
    return dwh, dbh, dw4, db4, dx3


def linear_fwd_slabs(xs, ws, ksplit=8, one_pass=False):
    """Raw split-K partial sums [nz][ksplit][B][O] of the fc4-shaped forward."""
    nz = len(xs)
    xs = [_c(x, _f32) for x in xs]
    ws = [_c(w, _f32) for w in ws]
    batch, fin = xs[0].shape
    fout = ws[0].shape[0]
    slabs = torch.full((nz, ksplit, batch, fout), float("nan"), dtype=_f32, device=xs[0].device)
    fn = lib.dra_linear_fwd_slabs_one if one_pass else lib.dra_linear_fwd_slabs
    fn(nz, ptr_array(xs), ptr_array(ws), batch, fin, fout, ksplit, ptr(slabs), stream_ptr())
    return slabs


class FoldSeg(ctypes.Structure):
    """Mirror of dra_fold_seg."""
    _fields_ = [("begin", ctypes.c_int64), ("count", ctypes.c_int64), ("slabs", ctypes.c_void_p),
                ("slab_stride", ctypes.c_int64), ("n_slabs", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def grad_sqnorm_segs(grad, segs, partials):
    """segs: list of (begin, count, slabs_tensor, slab_stride, n_slabs).  Returns the number of partials written."""
    arr = _fold_seg_array(segs)
    n = ctypes.c_int(0)
    lib.dra_grad_sqnorm_segs(ptr(grad), grad.numel(), arr, len(segs), ptr(partials), ctypes.byref(n), stream_ptr())
    return n.value


MAX_FOLD_SEGS = 4      # DRA_MAX_FOLD_SEGS (include/deeprl_amd.h)


def norm_partials_max():
    return lib.dra_norm_partials_max.raw()


def _fold_seg_array(segs):
    arr = (FoldSeg * max(1, len(segs)))()
    for i, (b, c, t, st, ns) in enumerate(segs):
        arr[i].begin, arr[i].count, arr[i].slabs, arr[i].slab_stride, arr[i].n_slabs = b, c, t.data_ptr(), st, ns
    return arr


def conv_bwd_x(layer, dy, w, xact=None, act="relu"):
    """Gradient w.r.t. the layer's input; with `xact` (the layer-below's activated output) the
    activation derivative of that layer is folded in (gradient w.r.t. its PRE-activation)."""
    c, h, oc, k, s = _CONV_GEOM[layer]
    batch = dy.shape[0]
    dx = torch.empty((batch, c, h, h), dtype=_f32, device=dy.device)
    lib.dra_conv_bwd_x(layer, ptr(_c(dy, _f32)), ptr(_c(w, _f32)), ptr(None if xact is None else _c(xact, _f32)), ptr(dx),
                       batch, ACT[act], stream_ptr())
    return dx


def act_bwd(dy, y, act):
    """dpre = dy * act'(y) (activation derivative through its output)."""
    dy, y = _c(dy, _f32), _c(y, _f32)
    out = torch.empty_like(dy)
    lib.dra_act_bwd(ptr(dy), ptr(y), ptr(out), dy.numel(), ACT[act], stream_ptr())
    return out


_ws_cache = {}


def _workspace(device, floats):
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    t = _ws_cache.get(key)
    if t is None or t.numel() < floats:
        t = torch.empty(max(floats, 1 << 20), dtype=_f32, device=device)
        _ws_cache[key] = t
    return t


def linear_fwd_pair(x, w0, b0, w1, b1, act=None):
    """(x W0^T + b0, x W1^T + b1) in one launch (two heads on the same features; in_features <= 512)."""
    x, w0, w1 = _c(x, _f32), _c(w0, _f32), _c(w1, _f32)
    b0 = None if b0 is None else _c(b0, _f32)
    b1 = None if b1 is None else _c(b1, _f32)
    batch, fin = x.shape
    y0 = torch.empty((batch, w0.shape[0]), dtype=_f32, device=x.device)
    y1 = torch.empty((batch, w1.shape[0]), dtype=_f32, device=x.device)
    lib.dra_linear_fwd_pair(ptr(x), ptr(w0), ptr(b0), ptr(y0), int(w0.shape[0]), ptr(w1), ptr(b1), ptr(y1), int(w1.shape[0]),
                            batch, fin, ACT[act], stream_ptr())
    return y0, y1


def gather_rows(tensors, idx):
    """[t[idx] for t in tensors] (row gathers along dim 0 of contiguous device tensors that share their row count) in ONE launch."""
    idx = _c(idx, torch.int64)
    n = int(idx.numel())
    k = len(tensors)
    if not 1 <= k <= 8:
        raise ValueError("gather_rows: 1..8 tensors")
    rows = int(tensors[0].shape[0])
    srcs, outs = [], []
    for t in tensors:
        t = _c(t)
        if t.dim() < 1 or int(t.shape[0]) != rows:
            raise ValueError("gather_rows: tensors must share dim 0")
        srcs.append(t)
        outs.append(torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device))
    src_arr = (ctypes.c_void_p * k)(*[t.data_ptr() for t in srcs])
    dst_arr = (ctypes.c_void_p * k)(*[t.data_ptr() for t in outs])
    rb = (ctypes.c_int64 * k)(*[(t.numel() // rows) * t.element_size() for t in srcs])
    lib.dra_gather_rows(k, src_arr, dst_arr, rb, ptr(idx), n, rows, stream_ptr())
    return outs


def policy_heads_sample(x, w0, b0, w1, b1, uniform, out=None):
    """A rollout step's policy head in one launch: (action i64 [B], log_pi_a [B], entropy [B], v [B]) of
    Categorical(logits = x W0^T + b0) sampled by inverse CDF from uniform [B], v = x w1^T + b1 -- linear_fwd_pair +
    categorical_fwd, bit for bit.  out: four preallocated tensors of those shapes (rows of a rollout's buffers)."""
    x, w0, w1, uniform = _c(x, _f32), _c(w0, _f32), _c(w1, _f32), _c(uniform, _f32)
    b0 = None if b0 is None else _c(b0, _f32)
    b1 = None if b1 is None else _c(b1, _f32)
    batch, fin = x.shape
    if w1.shape[0] != 1 or uniform.numel() != batch:
        raise ValueError("policy_heads_sample: one value output and one uniform per row")
    if out is None:
        out = (torch.empty(batch, dtype=torch.int64, device=x.device), torch.empty(batch, dtype=_f32, device=x.device),
               torch.empty(batch, dtype=_f32, device=x.device), torch.empty(batch, dtype=_f32, device=x.device))
    a, lp, ent, v = out
    for t_, dt in ((a, torch.int64), (lp, _f32), (ent, _f32), (v, _f32)):
        if t_.dtype != dt or t_.numel() != batch or not t_.is_contiguous():
            raise ValueError("policy_heads_sample: output rows must be contiguous [B] tensors (i64, f32, f32, f32)")
    lib.dra_policy_heads_sample(ptr(x), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(uniform), batch, fin, int(w0.shape[0]), ptr(a),
                                ptr(lp), ptr(ent), ptr(v), None, stream_ptr())
    return a, lp, ent, v


def policy_heads_given(x, w0, b0, w1, b1, action):
    """The update's forward through the policy head in one launch -> (log_pi_a [B], entropy [B], v [B], logits [B, A]) for the
    given actions (linear_fwd_pair + categorical_fwd(action=...), bit for bit)."""
    x, w0, w1, action = _c(x, _f32), _c(w0, _f32), _c(w1, _f32), _c(action, torch.int64)
    b0 = None if b0 is None else _c(b0, _f32)
    b1 = None if b1 is None else _c(b1, _f32)
    batch, fin = x.shape
    a = int(w0.shape[0])
    if w1.shape[0] != 1 or action.numel() != batch:
        raise ValueError("policy_heads_given: one value output and one action per row")
    lp, ent, v = (torch.empty(batch, dtype=_f32, device=x.device) for _ in range(3))
    logits = torch.empty((batch, a), dtype=_f32, device=x.device)
    lib.dra_policy_heads_given(ptr(x), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(action), batch, fin, a, ptr(lp), ptr(ent), ptr(v),
                               ptr(logits), stream_ptr())
    return lp, ent, v, logits


def fc4_policy_heads_given(y3, w4, b4, w0, b0, w1, b1, action):
    """fc4 (3136 -> 512, + ReLU) and the policy head for given actions as TWO launches: the one-pass K-slice forward (8 slabs) and
    the head launch that folds them -> (log_pi_a [B], entropy [B], v [B], logits [B, A], phi [B, 512]); linear_fwd + its finish +
    policy_heads_given were three, same arithmetic."""
    y3, w4, b4, w0, w1, action = _c(y3, _f32), _c(w4, _f32), _c(b4, _f32), _c(w0, _f32), _c(w1, _f32), _c(action, torch.int64)
    b0 = None if b0 is None else _c(b0, _f32)
    b1 = None if b1 is None else _c(b1, _f32)
    batch = int(y3.shape[0])
    a = int(w0.shape[0])
    dev = y3.device
    slabs = torch.empty((8, batch, 512), dtype=_f32, device=dev)      # (8 slices: the fastest at 80 / 256 rows, tools/fc4_small_probe.py)
    lib.dra_linear_fwd_slabs_one(1, ptr_array([y3]), ptr_array([w4]), batch, 3136, 512, 8, ptr(slabs), stream_ptr())
    lp, ent, v = (torch.empty(batch, dtype=_f32, device=dev) for _ in range(3))
    logits = torch.empty((batch, a), dtype=_f32, device=dev)
    phi = torch.empty((batch, 512), dtype=_f32, device=dev)
    lib.dra_policy_heads_given_fold(ptr(slabs), 8, ptr(b4), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(action), batch, a, ptr(lp),
                                      ptr(ent), ptr(v), ptr(logits), ptr(phi), stream_ptr())
    return lp, ent, v, logits, phi


def fc4_policy_heads_sample(y3, w4, b4, w0, b0, w1, b1, uniform, out=None):
    """fc4 (3136 -> 512, + ReLU) and the sampling policy head of a rollout step (<= 32 rows) as TWO launches: the one-pass K-slice
    forward with 28 slices and the head launch that folds them -> (action i64 [B], log_pi_a, entropy, v [B]).  (The eight-wave GEMV
    + policy_heads_sample are two as well, 5.6 / 8.1 / 13.2 + 6 us at 8 / 16 / 32 rows against 4.3 + 5: tools/fc4_small_probe.py.)"""
    y3, w4, b4, w0, w1, uniform = _c(y3, _f32), _c(w4, _f32), _c(b4, _f32), _c(w0, _f32), _c(w1, _f32), _c(uniform, _f32)
    b0 = None if b0 is None else _c(b0, _f32)
    b1 = None if b1 is None else _c(b1, _f32)
    batch = int(y3.shape[0])
    dev = y3.device
    slabs = torch.empty((28, batch, 512), dtype=_f32, device=dev)
    lib.dra_linear_fwd_slabs_one(1, ptr_array([y3]), ptr_array([w4]), batch, 3136, 512, 28, ptr(slabs), stream_ptr())
    if out is None:
        out = (torch.empty(batch, dtype=torch.int64, device=dev), torch.empty(batch, dtype=_f32, device=dev),
               torch.empty(batch, dtype=_f32, device=dev), torch.empty(batch, dtype=_f32, device=dev))
    a, lp, ent, v = out
    lib.dra_policy_heads_sample_fold28(ptr(slabs), ptr(b4), ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(uniform), batch, int(w0.shape[0]),
                                       ptr(a), ptr(lp), ptr(ent), ptr(v), stream_ptr())
    return a, lp, ent, v


def _check_rows(name, batch, **tensors):
    for k, (t, dt, n) in tensors.items():
        if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous() or not t.is_cuda):
            raise ValueError("%s: %s must be a contiguous device %s tensor of %d elements" % (name, k, dt, n))


def q_heads_fold28(slabs, fold_bias, w, b, explore=None, random_action=None, out_q=None, out_action=None, out_phi=None,
                   out_max=None):
    """The Q head of an n-step DQN rollout step on fc4's 28 K-slice partial sums slabs [28, B, 512] in one launch (one workgroup
    per row): phi = relu(sum of slices + fold_bias) -> out_phi, q = phi W^T + b -> out_q [B, A], action = explore ? random_action :
    argmax q (first index of the maximum) -> out_action i64 [B], max_a q -> out_max [B].  Outputs are written in place."""
    slabs, fold_bias, w = _c(slabs, _f32), _c(fold_bias, _f32), _c(w, _f32)
    b = None if b is None else _c(b, _f32)
    batch, a = int(slabs.shape[1]), int(w.shape[0])
    if tuple(slabs.shape) != (28, batch, 512) or tuple(w.shape) != (a, 512):
        raise ValueError("q_heads_fold28: slabs [28, B, 512], w [A, 512]")
    _check_rows("q_heads_fold28", batch, explore=(explore, torch.uint8, batch), random_action=(random_action, torch.int64, batch),
                out_q=(out_q, _f32, batch * a), out_action=(out_action, torch.int64, batch), out_phi=(out_phi, _f32, batch * 512),
                out_max=(out_max, _f32, batch))
    lib.dra_q_heads_fold28(ptr(slabs), ptr(fold_bias), ptr(w), ptr(b), ptr(explore), ptr(random_action), batch, a, ptr(out_q),
                           ptr(out_action), ptr(out_phi), ptr(out_max), stream_ptr())


def rollout_conv1_qheads(frames_u8, w1_koc, b1, y1, u8_coef, slabs_prev=None, fold_bias=None, w=None, b=None, explore=None,
                         random_action=None, out_q=None, out_action=None, out_phi=None):
    """conv1 (+ ReLU) of uint8 frames [B, 4, 84, 84] into y1 [B, 32, 20, 20] and -- slabs_prev given -- the previous step's Q head
    (q_heads_fold28's q / action / phi outputs) in the same launch."""
    batch = int(frames_u8.shape[0])
    a = 0 if w is None else int(w.shape[0])
    if frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous() or not y1.is_contiguous():
        raise ValueError("rollout_conv1_qheads: contiguous uint8 frames and f32 output")
    if slabs_prev is not None:
        _check_rows("rollout_conv1_qheads", batch, slabs_prev=(slabs_prev, _f32, 28 * batch * 512), fold_bias=(fold_bias, _f32, 512),
                    w=(w, _f32, a * 512), explore=(explore, torch.uint8, batch), random_action=(random_action, torch.int64, batch),
                    out_q=(out_q, _f32, batch * a), out_action=(out_action, torch.int64, batch), out_phi=(out_phi, _f32, batch * 512))
    lib.dra_rollout_conv1_qheads(ptr(frames_u8), ptr(w1_koc), ptr(b1), ptr(y1), batch, float(u8_coef), ptr(slabs_prev), ptr(fold_bias),
                                 ptr(w), ptr(b), ptr(explore), ptr(random_action), a, ptr(out_q), ptr(out_action), ptr(out_phi),
                                 stream_ptr())


def nstep_q_loss_bwd(q, action, reward, mask, bootstrap, gamma, phi, w, out=None):
    """NStepDQN_agent.py:56-67's returns, loss and the Q head's backward in ONE launch: q [T, N, A], action i64 [T, N], reward /
    mask [T, N] (any trailing 1), bootstrap [N], phi [T * N, 512], w [A, 512] -> dict(ret [T, N], loss [1], dw [A, 512], db [A],
    dphi [T * N, 512] (times fc4's ReLU mask)).  out: the same dict of preallocated tensors (dw / db may be gradient slots)."""
    q, action, phi, w = _c(q, _f32), _c(action, torch.int64), _c(phi, _f32), _c(w, _f32)
    reward, mask, bootstrap = _c(reward, _f32), _c(mask, _f32), _c(bootstrap, _f32)
    t_len, n, a = int(q.shape[0]), int(q.shape[1]), int(q.shape[2])
    rows = t_len * n
    if (action.numel() != rows or reward.numel() != rows or mask.numel() != rows or bootstrap.numel() != n
            or tuple(phi.shape) != (rows, 512) or tuple(w.shape) != (a, 512)):
        raise ValueError("nstep_q_loss_bwd: inconsistent shapes")
    dev = q.device
    if out is None:
        out = dict(ret=torch.empty((t_len, n), dtype=_f32, device=dev), loss=torch.empty(1, dtype=_f32, device=dev),
                   dw=torch.empty((a, 512), dtype=_f32, device=dev), db=torch.empty(a, dtype=_f32, device=dev),
                   dphi=torch.empty((rows, 512), dtype=_f32, device=dev))
    _check_rows("nstep_q_loss_bwd", rows, ret=(out['ret'], _f32, rows), loss=(out['loss'], _f32, 1), dw=(out['dw'], _f32, a * 512),
                db=(out['db'], _f32, a), dphi=(out['dphi'], _f32, rows * 512))
    lib.dra_nstep_q_loss_bwd(ptr(q), ptr(action), ptr(reward), ptr(mask), ptr(bootstrap), float(gamma), ptr(phi), ptr(w), t_len, n, a,
                             ptr(out['ret']), ptr(out['loss']), ptr(out['dw']), ptr(out['db']), ptr(out['dphi']), stream_ptr())
    return out


def _oc_head_checks(name, batch, n_opt, n_act, heads, uniform, eps, mask, prev_option, is_initial, out):
    if not (1 <= n_opt <= 8 and 1 <= n_act <= 18):
        raise ValueError("%s: at most 8 options and 18 actions" % name)
    wq, bq, wb, bb, wp, bp = heads
    i64, u8 = torch.int64, torch.uint8
    _check_rows(name, batch, w_q=(wq, _f32, n_opt * 512), b_q=(bq, _f32, n_opt), w_beta=(wb, _f32, n_opt * 512),
                b_beta=(bb, _f32, n_opt), w_pi=(wp, _f32, n_opt * n_act * 512), b_pi=(bp, _f32, n_opt * n_act),
                uniform=(uniform, _f32, batch * 3), eps=(eps, _f32, 1), mask=(mask, _f32, batch),
                prev_option=(prev_option, i64, batch), is_initial=(is_initial, is_initial.dtype if is_initial is not None else u8, batch))
    if is_initial is not None and is_initial.dtype not in (u8, torch.bool):
        raise ValueError("%s: is_initial must be uint8 or bool" % name)
    shapes = dict(q=(_f32, batch * n_opt), beta=(_f32, batch * n_opt), logits=(_f32, batch * n_act), option=(i64, batch),
                  action=(i64, batch), log_pi_a=(_f32, batch), entropy=(_f32, batch), prev_option=(i64, batch), init=(_f32, batch),
                  phi=(_f32, batch * 512), boot=(_f32, batch))
    unknown = set(out) - set(shapes)
    if unknown:
        raise ValueError("%s: unknown outputs %s" % (name, sorted(unknown)))
    _check_rows(name, batch, **{k: (v, shapes[k][0], shapes[k][1]) for k, v in out.items()})


def oc_heads_fold28(slabs, fold_bias, w_q, b_q, w_beta, b_beta, w_pi=None, b_pi=None, uniform=None, eps=None, mask=None,
                    prev_option=None, is_initial=None, out=None, boot=None):
    """The option-critic head of a rollout step on fc4's 28 K-slice partial sums slabs [28, B, 512] in one launch (one workgroup
    per row; rollout_roles.h oc_head_row_fold_wg): q [B, O], beta [B, O], the option (sample_option with this step's eps [1] and
    uniform [B, 3] columns fresh / continued), the action from the chosen option's policy, its logits [B, A], log pi(a), entropy
    and phi [B, 512].  prev_option i64 [B] and is_initial u8 / bool [B] are the carried state, replaced in place (prev <- option,
    init <- mask == 0); out: dict of preallocated outputs (any of q, beta, logits, option, action, log_pi_a, entropy, prev_option
    (what the step read), init (likewise, f32), phi), written in place.  boot [B] given: the bootstrap mode
    (OptionCritic_agent.py:87-93) -- q / beta of the target network and boot = (1 - beta[prev]) q[prev] + beta[prev] max q."""
    slabs, fold_bias = _c(slabs, _f32), _c(fold_bias, _f32)
    batch, n_opt = int(slabs.shape[1]), int(w_q.shape[0])
    n_act = int(w_pi.shape[0]) // n_opt if w_pi is not None else 1
    if tuple(slabs.shape) != (28, batch, 512):
        raise ValueError("oc_heads_fold28: slabs [28, B, 512]")
    if prev_option is None or (boot is None and (w_pi is None or uniform is None or eps is None or mask is None or is_initial is None)):
        raise ValueError("oc_heads_fold28: prev_option always; w_pi, uniform, eps, mask, is_initial outside the bootstrap mode")
    out = dict(out or {})
    if boot is not None:
        out['boot'] = boot
    _oc_head_checks("oc_heads_fold28", batch, n_opt, n_act, (w_q, b_q, w_beta, b_beta, w_pi, b_pi), uniform, eps, mask, prev_option,
                    is_initial, out)
    g = out.get
    lib.dra_oc_heads_fold28(ptr(slabs), ptr(fold_bias), ptr(w_q), ptr(b_q), ptr(w_beta), ptr(b_beta), ptr(w_pi), ptr(b_pi),
                            ptr(uniform), ptr(eps), ptr(mask), ptr(prev_option), ptr(is_initial), batch, n_opt, n_act, ptr(g('q')),
                            ptr(g('beta')), ptr(g('logits')), ptr(g('option')), ptr(g('action')), ptr(g('log_pi_a')),
                            ptr(g('entropy')), ptr(g('prev_option')), ptr(g('init')), ptr(g('phi')), ptr(g('boot')), stream_ptr())
    return out


def rollout_conv1_ocheads(frames_u8, w1_koc, b1, y1, u8_coef, slabs_prev=None, fold_bias=None, heads=None, uniform=None, eps=None,
                          mask=None, prev_option=None, is_initial=None, out=None):
    """conv1 (+ ReLU) of uint8 frames [B, 4, 84, 84] into y1 [B, 32, 20, 20] and -- slabs_prev given -- the previous step's
    option-critic head (oc_heads_fold28's decision mode; heads = (w_q, b_q, w_beta, b_beta, w_pi, b_pi)) in the same launch."""
    batch = int(frames_u8.shape[0])
    if frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous() or not y1.is_contiguous():
        raise ValueError("rollout_conv1_ocheads: contiguous uint8 frames and f32 output")
    out = dict(out or {})
    n_opt = n_act = 0
    heads = tuple(heads) if heads is not None else (None,) * 6
    if slabs_prev is not None:
        if any(x is None for x in (fold_bias, heads[0], heads[2], heads[4], uniform, eps, mask, prev_option, is_initial)):
            raise ValueError("rollout_conv1_ocheads: the head needs fold_bias, heads, uniform, eps, mask and the carried state")
        n_opt = int(heads[0].shape[0])
        n_act = int(heads[4].shape[0]) // n_opt
        _check_rows("rollout_conv1_ocheads", batch, slabs_prev=(slabs_prev, _f32, 28 * batch * 512), fold_bias=(fold_bias, _f32, 512))
        _oc_head_checks("rollout_conv1_ocheads", batch, n_opt, n_act, heads, uniform, eps, mask, prev_option, is_initial, out)
    g = out.get
    lib.dra_rollout_conv1_ocheads(ptr(frames_u8), ptr(w1_koc), ptr(b1), ptr(y1), batch, float(u8_coef), ptr(slabs_prev), ptr(fold_bias),
                                  *[ptr(x) for x in heads], ptr(uniform), ptr(eps), ptr(mask), ptr(prev_option), ptr(is_initial),
                                  n_opt, n_act, ptr(g('q')), ptr(g('beta')), ptr(g('logits')), ptr(g('option')), ptr(g('action')),
                                  ptr(g('log_pi_a')), ptr(g('entropy')), ptr(g('prev_option')), ptr(g('init')), ptr(g('phi')),
                                  stream_ptr())
    return out


_OC_LOSS_OUTS = ("ret", "adv", "beta_adv", "loss", "dw_q", "db_q", "dw_pi", "db_pi", "dw_beta", "db_beta", "dphi")


def oc_loss_bwd(rollout, reward, mask, ret_boot, eps, gamma, termination_regularizer, entropy_weight, phi, w_q, w_pi, w_beta,
                out=None):
    """OptionCritic_agent.py:95-117's returns, advantages, termination advantages, the three losses and the heads' backward in ONE
    launch.  rollout: dict of the head's outputs over T steps x N environments (q / beta [T, N, O], logits [T, N, A], option /
    action / prev_option i64 [T, N], init / log_pi_a / entropy [T, N]); reward / mask [T, N] (any trailing 1), ret_boot [N], eps
    [T]; phi [T * N, 512]; w_q / w_beta [O, 512], w_pi [O * A, 512] -> dict(ret, adv, beta_adv [T, N], loss [4] = (total, q, pi,
    beta), dw_q, db_q, dw_pi, db_pi, dw_beta, db_beta, dphi [T * N, 512] (times fc4's ReLU mask)).  out: the same dict of
    preallocated tensors (the weight gradients may be gradient slots)."""
    r = {k: _c(rollout[k], torch.int64 if k in ("option", "action", "prev_option") else _f32)
         for k in ("q", "beta", "logits", "option", "action", "prev_option", "init", "log_pi_a", "entropy")}
    reward, mask, ret_boot, eps, phi = _c(reward, _f32), _c(mask, _f32), _c(ret_boot, _f32), _c(eps, _f32), _c(phi, _f32)
    w_q, w_pi, w_beta = _c(w_q, _f32), _c(w_pi, _f32), _c(w_beta, _f32)
    t_len, n, n_opt = int(r['q'].shape[0]), int(r['q'].shape[1]), int(r['q'].shape[2])
    n_act = int(r['logits'].shape[-1])
    rows = t_len * n
    if not (1 <= n_opt <= 8 and 1 <= n_act <= 18) or rows > 2048:
        raise ValueError("oc_loss_bwd: at most 8 options, 18 actions and 2048 rows")
    if (r['beta'].numel() != rows * n_opt or r['logits'].numel() != rows * n_act
            or any(r[k].numel() != rows for k in ("option", "action", "prev_option", "init", "log_pi_a", "entropy"))
            or reward.numel() != rows or mask.numel() != rows or ret_boot.numel() != n or eps.numel() != t_len
            or tuple(phi.shape) != (rows, 512) or tuple(w_q.shape) != (n_opt, 512) or tuple(w_beta.shape) != (n_opt, 512)
            or tuple(w_pi.shape) != (n_opt * n_act, 512)):
        raise ValueError("oc_loss_bwd: inconsistent shapes")
    dev = phi.device
    shapes = dict(ret=(t_len, n), adv=(t_len, n), beta_adv=(t_len, n), loss=(4,), dw_q=(n_opt, 512), db_q=(n_opt,),
                  dw_pi=(n_opt * n_act, 512), db_pi=(n_opt * n_act,), dw_beta=(n_opt, 512), db_beta=(n_opt,), dphi=(rows, 512))
    if out is None:
        out = {k: torch.empty(s, dtype=_f32, device=dev) for k, s in shapes.items()}
    _check_rows("oc_loss_bwd", rows, **{k: (out[k], _f32, int(np.prod(s))) for k, s in shapes.items()})
    lib.dra_oc_loss_bwd(ptr(r['q']), ptr(r['beta']), ptr(r['logits']), ptr(r['option']), ptr(r['action']), ptr(r['prev_option']),
                        ptr(r['init']), ptr(r['log_pi_a']), ptr(r['entropy']), ptr(reward), ptr(mask), ptr(ret_boot), ptr(eps),
                        float(gamma), float(termination_regularizer), float(entropy_weight), ptr(phi), ptr(w_q), ptr(w_pi),
                        ptr(w_beta), t_len, n, n_opt, n_act, *[ptr(out[k]) for k in _OC_LOSS_OUTS], stream_ptr())
    return out


HEADS_BWD_MAX_BATCH = 8192


def policy_heads_bwd(logits, action, g_lp, g_ent, g_v, x, w0, w1, dw0=None, db0=None, dw1=None, db1=None, want_dx=True,
                     relu_mask=False):
    """Backward of policy_heads_given in one launch -> (dx or None, dw0, db0, dw1, db1); g_* [B] or None (= zero); dw / db may
    be given (written in place); relu_mask: x is a fused-ReLU output, dx is the gradient of its PRE-activation."""
    logits, action, x, w0, w1 = _c(logits, _f32), _c(action, torch.int64), _c(x, _f32), _c(w0, _f32), _c(w1, _f32)
    g_lp, g_ent, g_v = [None if g is None else _c(g, _f32) for g in (g_lp, g_ent, g_v)]
    batch, fin = x.shape
    a = int(w0.shape[0])
    dev = x.device
    dw0 = torch.empty((a, fin), dtype=_f32, device=dev) if dw0 is None else dw0
    db0 = torch.empty(a, dtype=_f32, device=dev) if db0 is None else db0
    dw1 = torch.empty((1, fin), dtype=_f32, device=dev) if dw1 is None else dw1
    db1 = torch.empty(1, dtype=_f32, device=dev) if db1 is None else db1
    dx = torch.empty((batch, fin), dtype=_f32, device=dev) if want_dx else None
    lib.dra_policy_heads_bwd(ptr(logits), ptr(action), ptr(g_lp), ptr(g_ent), ptr(g_v), ptr(x), ptr(w0), ptr(w1), ptr(dx), ptr(dw0),
                             ptr(db0), ptr(dw1), ptr(db1), batch, fin, a, 1 if relu_mask else 0, stream_ptr())
    return dx, dw0, db0, dw1, db1


def linear_bwd_pair(g0, g1, x, w0, w1, dw0=None, db0=None, dw1=None, db1=None, want_dx=True):
    """Backward of linear_fwd_pair in one launch -> (dx or None, dw0, db0, dw1, db1); dw / db may be given (written in place)."""
    g0, g1, x, w0, w1 = [_c(t, _f32) for t in (g0, g1, x, w0, w1)]
    batch, fin = x.shape
    o0, o1 = w0.shape[0], w1.shape[0]
    dev = x.device
    dw0 = torch.empty((o0, fin), dtype=_f32, device=dev) if dw0 is None else dw0
    db0 = torch.empty(o0, dtype=_f32, device=dev) if db0 is None else db0
    dw1 = torch.empty((o1, fin), dtype=_f32, device=dev) if dw1 is None else dw1
    db1 = torch.empty(o1, dtype=_f32, device=dev) if db1 is None else db1
    dx = torch.empty((batch, fin), dtype=_f32, device=dev) if want_dx else None
    lib.dra_linear_bwd_pair(ptr(g0), ptr(g1), ptr(x), ptr(w0), ptr(w1), ptr(dx), ptr(dw0), ptr(db0), ptr(dw1), ptr(db1), batch, fin,
                            o0, o1, stream_ptr())
    return dx, dw0, db0, dw1, db1


def linear_fwd(xs, ws, bs, act=None):
    nz = len(xs)
    xs = [_c(x, _f32) for x in xs]
    batch, fin = xs[0].shape
    fout = ws[0].shape[0]
    ws = [_c(w, _f32) for w in ws]
    bs = [None if b is None else _c(b, _f32) for b in bs]
    ys = [torch.empty((batch, fout), dtype=_f32, device=xs[0].device) for _ in range(nz)]
    need = nz * 32 * batch * fout
    wsb = _workspace(xs[0].device, need)
    lib.dra_linear_fwd(nz, ptr_array(xs), ptr_array(ws), ptr_array(bs), ptr_array(ys), batch, fin, fout, ACT[act],
                       ptr(wsb), wsb.numel(), stream_ptr())
    return ys


def linear_bwd_w(dy, x, dw=None, db=None, want_bias=True):
    dy, x = _c(dy, _f32), _c(x, _f32)
    batch, fout = dy.shape
    fin = x.shape[1]
    if dw is None:
        dw = torch.empty((fout, fin), dtype=_f32, device=x.device)
    if db is None and want_bias:
        db = torch.empty(fout, dtype=_f32, device=x.device)
    lib.dra_linear_bwd_w(ptr(dy), ptr(x), ptr(dw), ptr(db), batch, fin, fout, stream_ptr())
    return dw, db


def linear_bwd_xw_512(dy, x, w, x_relu, dw=None, db=None, want_bias=True):
    """Input gradient and weight / bias gradient of a 512-output layer with in_features >= 1024 in ONE launch -> (dx, dw, db):
    linear_bwd_x(dy, w, xact=x if x_relu, act='relu') and linear_bwd_w(dy, x), same arithmetic."""
    dy, x, w = _c(dy, _f32), _c(x, _f32), _c(w, _f32)
    batch, fin = x.shape
    if dw is None:
        dw = torch.empty((512, fin), dtype=_f32, device=x.device)
    if db is None and want_bias:
        db = torch.empty(512, dtype=_f32, device=x.device)
    dx = torch.empty((batch, fin), dtype=_f32, device=x.device)
    lib.dra_linear_bwd_xw_one512(ptr(dy), ptr(w), ptr(x), 1 if x_relu else 0, ptr(dx), ptr(dw), ptr(db), batch, fin, stream_ptr())
    return dx, dw, db


def linear_bwd_x(dy, w, xact=None, act=None, dx=None):
    dy, w = _c(dy, _f32), _c(w, _f32)
    batch, fout = dy.shape
    fin = w.shape[1]
    if dx is None:
        dx = torch.empty((batch, fin), dtype=_f32, device=dy.device)
    lib.dra_linear_bwd_x(ptr(dy), ptr(w), ptr(None if xact is None else _c(xact, _f32)), ptr(dx), batch, fin, fout,
                         ACT[act], stream_ptr())
    return dx


# ------------------------------------------------------------------------------------------ noisy layers (csrc/noisy.hip)
_noisy_ws_need = {}


def _noisy_workspace(device, rows, fin, fout, which):
    need = _noisy_ws_need.get((rows, fin, fout))
    if need is None:
        f, b = ctypes.c_int64(0), ctypes.c_int64(0)
        lib.dra_noisy_workspace_floats(rows, fin, fout, ctypes.byref(f), ctypes.byref(b))
        need = _noisy_ws_need[(rows, fin, fout)] = (f.value, b.value)
    return _workspace(device, need[which])


def noisy_linear_fwd(x, w_mu, w_sigma, b_mu, b_sigma, noise_in, noise_out_weight, noise_out_bias, act=None):
    """y = act(x W^T + b) of a NoisyLinear layer (network_utils.py:54-62) from the raw noise vectors; the mixed weight is never
    formed.  x [rows <= 1024, in], w_* [out, in]."""
    x, w_mu, w_sigma = _c(x, _f32), _c(w_mu, _f32), _c(w_sigma, _f32)
    rows, fin = x.shape
    fout = w_mu.shape[0]
    if w_mu.shape != (fout, fin) or w_sigma.shape != (fout, fin) or noise_in.numel() != fin or noise_out_weight.numel() != fout \
            or noise_out_bias.numel() != fout or b_mu.numel() != fout or b_sigma.numel() != fout:
        raise DraError("noisy_linear_fwd: shapes do not agree")
    y = torch.empty((rows, fout), dtype=_f32, device=x.device)
    ws = _noisy_workspace(x.device, rows, fin, fout, 0)
    lib.dra_noisy_linear_fwd(ptr(x), ptr(w_mu), ptr(w_sigma), ptr(_c(b_mu, _f32)), ptr(_c(b_sigma, _f32)), ptr(_c(noise_in, _f32)),
                             ptr(_c(noise_out_weight, _f32)), ptr(_c(noise_out_bias, _f32)), ptr(y), rows, fin, fout, ACT[act],
                             ptr(ws), ws.numel(), stream_ptr())
    return y


def noisy_linear_fwd_rows(x, w_mu, w_sigma, b_mu, b_sigma, noise_in, noise_out_weight, noise_out_bias, act=None, out=None):
    """noisy_linear_fwd for the rows <= 8 transitions of one agent step, row r under its own noise draw: noise_in [rows, in],
    noise_out_weight / noise_out_bias [rows, out] -- dense, or three column slices of ONE [rows, numel] block (nets._NoiseBlock.
    draw_rows).  Row r has the bits of noisy_linear_fwd(x[r:r + 1], ..., noise row r)."""
    x, w_mu, w_sigma = _c(x, _f32), _c(w_mu, _f32), _c(w_sigma, _f32)
    rows, fin = x.shape
    fout = w_mu.shape[0]
    if w_mu.shape != (fout, fin) or w_sigma.shape != (fout, fin) or b_mu.numel() != fout or b_sigma.numel() != fout \
            or tuple(noise_in.shape) != (rows, fin) or tuple(noise_out_weight.shape) != (rows, fout) \
            or tuple(noise_out_bias.shape) != (rows, fout):
        raise DraError("noisy_linear_fwd_rows: shapes do not agree")
    noise = (noise_in, noise_out_weight, noise_out_bias)
    for e in noise:
        _dev(e)
        if e.dtype != _f32 or e.stride(1) != 1:
            raise DraError("noisy_linear_fwd_rows: noise rows must be contiguous f32")
    if all(e.is_contiguous() for e in noise):
        stride = 0
    else:
        stride = noise_in.stride(0) if rows > 1 else max(fin, fout)
        if rows > 1 and any(e.stride(0) != stride for e in noise):
            raise DraError("noisy_linear_fwd_rows: the three noise blocks must share one row stride")
    y = torch.empty((rows, fout), dtype=_f32, device=x.device) if out is None else out
    lib.dra_noisy_linear_fwd_rows(ptr(x), ptr(w_mu), ptr(w_sigma), ptr(_c(b_mu, _f32)), ptr(_c(b_sigma, _f32)), ptr(noise_in),
                                  ptr(noise_out_weight), ptr(noise_out_bias), int(stride), ptr(y), rows, fin, fout, ACT[act],
                                  stream_ptr())
    return y


def rainbow_act_rows(value, advantage, atoms, want_q=False, action=None):
    """Greedy actions of rows <= 8 Rainbow forwards in one launch: dueling combination, softmax over the atoms, expected value,
    first maximum.  value [rows, Z], advantage [rows, A, Z], atoms [Z]; -> (action int64 [rows] -- `action` when given --, q [rows, A]
    or None)."""
    value, advantage, atoms = _c(value, _f32), _c(advantage, _f32), _c(atoms, _f32)
    b, a, z = advantage.shape
    if value.shape != (b, z) or atoms.numel() != z:
        raise DraError("rainbow_act_rows: value %s / atoms %d do not fit advantage %s" % (tuple(value.shape), atoms.numel(),
                                                                                         tuple(advantage.shape)))
    if action is None:
        action = torch.empty(b, dtype=torch.int64, device=value.device)
    elif action.dtype != torch.int64 or action.numel() != b or not action.is_contiguous():
        raise DraError("rainbow_act_rows: action must be a contiguous int64 tensor of %d elements" % b)
    q = torch.empty((b, a), dtype=_f32, device=value.device) if want_q else None
    lib.dra_rainbow_act_rows(ptr(value), ptr(advantage), ptr(atoms), b, a, z, ptr(_dev(action)), ptr(q), stream_ptr())
    return action, q


def noisy_linear_bwd(g, x, w_mu, w_sigma, noise_in, noise_out_weight, noise_out_bias, x_relu=False, want_dx=True, dw_mu=None,
                     dw_sigma=None, db_mu=None, db_sigma=None, dx_add=None):
    """Backward of noisy_linear_fwd from g = dL/d(pre-activation) -> (dx, dw_mu, dw_sigma, db_mu, db_sigma); the four parameter
    gradients go into the given (contiguous) tensors when all four are passed.  dx_add [rows, in]: added to dx (the input gradient
    of another head on the same features).  x_relu: x is a fused-ReLU output, dx comes back as the gradient of its
    pre-activation."""
    g, x, w_mu, w_sigma = _c(g, _f32), _c(x, _f32), _c(w_mu, _f32), _c(w_sigma, _f32)
    rows, fin = x.shape
    fout = w_mu.shape[0]
    if g.shape != (rows, fout) or w_mu.shape != (fout, fin) or w_sigma.shape != (fout, fin):
        raise DraError("noisy_linear_bwd: shapes do not agree")
    dev = x.device
    if dw_mu is None:
        dw_mu, dw_sigma = torch.empty((fout, fin), dtype=_f32, device=dev), torch.empty((fout, fin), dtype=_f32, device=dev)
        db_mu, db_sigma = torch.empty(fout, dtype=_f32, device=dev), torch.empty(fout, dtype=_f32, device=dev)
    dx = torch.empty((rows, fin), dtype=_f32, device=dev) if want_dx else None
    ws = _noisy_workspace(dev, rows, fin, fout, 1)
    lib.dra_noisy_linear_bwd(ptr(g), ptr(x), ptr(w_mu), ptr(w_sigma), ptr(_c(noise_in, _f32)), ptr(_c(noise_out_weight, _f32)),
                             ptr(_c(noise_out_bias, _f32)), ptr(x if (x_relu and want_dx) else None),
                             ptr(None if (dx_add is None or not want_dx) else _c(dx_add, _f32)), ptr(dw_mu), ptr(dw_sigma),
                             ptr(db_mu), ptr(db_sigma), ptr(dx), rows, fin, fout, ptr(ws), ws.numel(), stream_ptr())
    return dx, dw_mu, dw_sigma, db_mu, db_sigma


def dueling_atoms_fwd(value, advantage):
    """logits[b, a, :] = value[b, :] + (advantage[b, a, :] - mean_a advantage[b, :, :]) (network_heads.py:79-86); value [B, Z],
    advantage [B, A, Z]."""
    value, advantage = _c(value, _f32), _c(advantage, _f32)
    b, a, z = advantage.shape
    if value.shape != (b, z):
        raise DraError("dueling_atoms_fwd: value %s does not fit advantage %s" % (tuple(value.shape), tuple(advantage.shape)))
    out = torch.empty_like(advantage)
    lib.dra_dueling_atoms_fwd(ptr(value), ptr(advantage), b, a, z, ptr(out), stream_ptr())
    return out


def dueling_atoms_bwd(g_logits):
    """(d_value [B, Z], d_advantage [B, A, Z]) of dueling_atoms_fwd."""
    g = _c(g_logits, _f32)
    b, a, z = g.shape
    dv = torch.empty((b, z), dtype=_f32, device=g.device)
    da = torch.empty_like(g)
    lib.dra_dueling_atoms_bwd(ptr(g), b, a, z, ptr(dv), ptr(da), stream_ptr())
    return dv, da


def per_weights_dev(loss_vec, sampling_prob, beta_dev, replay_eps, replay_alpha, prio=None, w=None):
    """per_weights with the importance exponent in a device word (beta_dev: f32 tensor of one element): no per-update launch
    argument, so the launch can be captured."""
    sp = _c(sampling_prob, _f32)
    b = sp.numel()
    if beta_dev.dtype != _f32 or beta_dev.numel() < 1:
        raise DraError("per_weights_dev: beta_dev must hold one f32")
    if prio is None and loss_vec is not None:
        prio = torch.empty(b, dtype=_f32, device=sp.device)
    if w is None:
        w = torch.empty(b, dtype=_f32, device=sp.device)
    lib.dra_per_weights_dev(ptr(None if loss_vec is None else _c(loss_vec, _f32)), ptr(sp), b, ptr(_dev(beta_dev)),
                            float(replay_eps), float(replay_alpha), ptr(prio), ptr(w), stream_ptr())
    return prio, w


# ------------------------------------------------------------------------------------------ optimiser
def norm_partials():
    return lib.dra_norm_partials.raw()


def grad_sqnorm(grad, partials, slabs=None, n_slabs=0, slab_stride=0):
    lib.dra_grad_sqnorm(ptr(grad), grad.numel(), ptr(slabs), int(n_slabs), int(slab_stride), ptr(partials), stream_ptr())


def rmsprop_step(param, grad, square_avg, grad_avg, partials, n_partials, max_norm, lr, alpha, eps, centered,
                 out_norm=None, param_copy=None):
    """param_copy (optional): the updated parameters are also written there (dra_rmsprop_step_copy)."""
    if param_copy is not None:
        lib.dra_rmsprop_step_copy(ptr(param), ptr(grad), ptr(square_avg), ptr(grad_avg), param.numel(), ptr(partials),
                                  int(n_partials), float(max_norm if max_norm else 0.0), float(lr), float(alpha), float(eps),
                                  int(bool(centered)), ptr(out_norm), ptr(param_copy), stream_ptr())
        return
    lib.dra_rmsprop_step(ptr(param), ptr(grad), ptr(square_avg), ptr(grad_avg), param.numel(), ptr(partials),
                         int(n_partials), float(max_norm if max_norm else 0.0), float(lr), float(alpha), float(eps),
                         int(bool(centered)), ptr(out_norm), stream_ptr())


def fc4_rider_step(param, grad, square_avg, grad_avg, param_copy, begin4, count4, coef, pending, lr, alpha, eps, centered,
                   write_through):
    """The deferred fc4 step's rider code alone, as one launch (dra_fc4_rider_test, a test aid): float4s [begin4, begin4 +
    count4) of the flat buffers are stepped if the device int32 `pending` is non-zero.  write_through: the form the chained
    forward launch carries, else the plain form of the flush; coef: device f32 clip coefficient; param_copy may be None."""
    lib.dra_fc4_rider_test(ptr(param), ptr(grad), ptr(square_avg), ptr(grad_avg), ptr(param_copy), int(begin4), int(count4),
                           ptr(coef), ptr(pending), float(lr), float(alpha), float(eps), int(bool(centered)),
                           int(bool(write_through)), stream_ptr())


OPT_RMSPROP, OPT_ADAM = 0, 1      # DRA_OPT_RMSPROP / DRA_OPT_ADAM (include/deeprl_amd.h)


def clip_step_late_blocks(seg):
    """seg: (begin, count, slabs_tensor, slab_stride, n_slabs).  Fold workgroups (= slots published) of clip_step_late:
    pure host arithmetic."""
    n = ctypes.c_int(0)
    lib.dra_clip_step_late_blocks(_fold_seg_array([seg]), ctypes.byref(n))
    return n.value


def clip_step_late(param, grad, state1, state2, seg, partials, n_prior, timeout_flag, optimizer, max_norm, hyper, centered,
                   step_dev=None, out_norm=None, param_copy=None):
    """The late-fold optimizer launch (dra_clip_step_late): folds `seg` (the one segment still in slabs, from element 0),
    publishes its sums of squares into partials[n_prior, n_prior + clip_step_late_blocks(seg)) -- which must hold -1.0 at
    launch -- and steps.  optimizer: OPT_RMSPROP with hyper = (lr, alpha, eps) or OPT_ADAM with hyper = (lr, beta1, eps,
    beta2) and the int64 device tensor `step_dev`; timeout_flag: a pinned host int32 tensor (non-zero afterwards: a
    bounded device-side wait gave up, the results are invalid)."""
    if timeout_flag.is_cuda or not timeout_flag.is_pinned() or timeout_flag.dtype != torch.int32:
        raise DraError("clip_step_late: timeout_flag must be a pinned host int32 tensor")
    hyper = tuple(float(h) for h in hyper)
    hp = (ctypes.c_float * 4)(*(hyper + (0.0,) * (4 - len(hyper))))
    lib.dra_clip_step_late(ptr(param), ptr(grad), ptr(state1), ptr(state2), param.numel(), _fold_seg_array([seg]),
                           ptr(partials), int(n_prior), ptr(timeout_flag), int(optimizer), float(max_norm if max_norm else 0.0),
                           hp, int(bool(centered)), ptr(step_dev), ptr(out_norm), ptr(param_copy), stream_ptr())


def adam_step(param, grad, exp_avg, exp_avg_sq, partials, n_partials, max_norm, lr, beta1, beta2, eps, step,
              out_norm=None):
    lib.dra_adam_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), ptr(partials),
                      int(n_partials), float(max_norm if max_norm else 0.0), float(lr), float(beta1), float(beta2),
                      float(eps), int(step), ptr(out_norm), stream_ptr())


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, partials, n_partials, max_norm, beta1, beta2, eps, hyper_dev,
                  out_norm=None):
    """Adam with {lr/(1-b1^t), 1/sqrt(1-b2^t)} read from the device tensor `hyper_dev` (graph-replayable)."""
    lib.dra_adam_step_dev(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), ptr(partials),
                          int(n_partials), float(max_norm if max_norm else 0.0), float(beta1), float(beta2), float(eps),
                          ptr(hyper_dev), ptr(out_norm), stream_ptr())


def categorical_fwd(logits, action=None, uniform=None):
    """Categorical(logits): (action, log_pi_a [B], entropy [B]); action None -> sampled by inverse CDF from `uniform` [B]."""
    logits = _c(logits, _f32)
    b, a = logits.shape
    lp = torch.empty(b, dtype=_f32, device=logits.device)
    ent = torch.empty(b, dtype=_f32, device=logits.device)
    if action is None:
        out_a = torch.empty(b, dtype=torch.int64, device=logits.device)
        lib.dra_categorical_fwd(ptr(logits), b, a, None, ptr(_c(uniform, _f32)), ptr(out_a), ptr(lp), ptr(ent), stream_ptr())
        return out_a, lp, ent
    action = _c(action, torch.int64)
    lib.dra_categorical_fwd(ptr(logits), b, a, ptr(action), None, None, ptr(lp), ptr(ent), stream_ptr())
    return action, lp, ent


class PerChain2IO(ctypes.Structure):
    """include/deeprl_amd.h dra_per_chain2_io (pinned host block of one dra_sumtree_per_chain2 launch)."""
    _fields_ = [("add_n", ctypes.c_int32), ("batch", ctypes.c_int32), ("next_batch", ctypes.c_int32), ("force_ordered", ctypes.c_int32),
                ("history", ctypes.c_int32), ("n_step", ctypes.c_int32), ("add_write0", ctypes.c_int64),
                ("memory_size", ctypes.c_int64), ("pos_after", ctypes.c_int64), ("size_after", ctypes.c_int64),
                ("rng_produced", ctypes.c_uint64), ("beta_next", ctypes.c_float), ("reserved", ctypes.c_int32),
                ("out_raw_idx", ctypes.c_int64 * 1024), ("out_idx", ctypes.c_int64 * 1024), ("out_p", ctypes.c_double * 1024),
                ("out_total", ctypes.c_double), ("out_n_valid", ctypes.c_int32), ("out_flags", ctypes.c_int32),
                ("out_rng_cursor", ctypes.c_uint64), ("out_seq", ctypes.c_uint64)]


PER_RNG_WORDS = 65536     # include/deeprl_amd.h DRA_PER_RNG_WORDS


class AtariPreprocess:
    """envs.py:39-47 (baselines' MaxAndSkipEnv max + WarpFrame: RGB2GRAY, INTER_AREA resize to 84x84) as one kernel
    (csrc/preproc.hip): raw [n_env][2][H][W][3] uint8 (the last two frames of each environment's frame skip; host array or
    device tensor) -> device uint8 [n_env][84][84], what FrameStack / the replay ring take.  The two axis tables are built
    once on the host by dra_resize_area_tab (OpenCV's computeResizeAreaTab)."""

    def __init__(self, height=210, width=160, out_h=84, out_w=84, device=None):
        from .support import Config
        self.h, self.w, self.oh, self.ow = int(height), int(width), int(out_h), int(out_w)
        self.device = device or Config.DEVICE
        self.tabs = []
        for ssize, dsize in ((self.w, self.ow), (self.h, self.oh)):
            cap = 2 * ssize + dsize + 8
            si, al, off = (ctypes.c_int * cap)(), (ctypes.c_float * cap)(), (ctypes.c_int * (dsize + 1))()
            n = lib.dra_resize_area_tab.raw(ssize, dsize, si, al, off, cap)
            if n <= 0:
                raise DraError("dra_resize_area_tab(%d, %d) failed: %d" % (ssize, dsize, n))
            self.tabs += [torch.tensor(list(si[:n]), dtype=torch.int32, device=self.device),
                          torch.tensor(list(al[:n]), dtype=torch.float32, device=self.device),
                          torch.tensor(list(off), dtype=torch.int32, device=self.device)]

    def __call__(self, raw2, out=None):
        if not isinstance(raw2, torch.Tensor):
            raw2 = torch.from_numpy(np.ascontiguousarray(raw2, dtype=np.uint8)).to(self.device, non_blocking=True)
        raw2 = _c(raw2, torch.uint8)
        n = raw2.shape[0]
        if tuple(raw2.shape[1:]) != (2, self.h, self.w, 3):
            raise DraError("AtariPreprocess: raw frames must be [n_env, 2, %d, %d, 3] uint8" % (self.h, self.w))
        if out is None:
            out = torch.empty((n, self.oh, self.ow), dtype=torch.uint8, device=raw2.device)
        t = self.tabs
        lib.dra_atari_preprocess(ptr(raw2), n, self.h, self.w, self.oh, self.ow, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]),
                                 ptr(t[5]), ptr(out), stream_ptr())
        return out


def gumbel_sample(logits, seed, step_dev, lo):
    """Rank-invariant categorical sample (dra_gumbel_sample): noise hashed from (seed, *step_dev, global row lo + i, action);
    advances the device step counter.  Graph-capturable (no host-side generator)."""
    logits = _c(logits, _f32)
    b, a = logits.shape
    out = torch.empty(b, dtype=torch.int64, device=logits.device)
    lib.dra_gumbel_sample(ptr(logits), b, a, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step_dev), int(lo), ptr(out), stream_ptr())
    return out


def cartpole_step(state, counter, ep_steps, ep_return, seed, action, horizon):
    """One step of n device-resident cart-pole environments with auto reset (dra_cartpole_step; csrc/cartpole_env.h): state f64
    [n, 4], counter i64 [n], ep_steps i32 [n] and ep_return f64 [n] are updated in place; action i64 [n] -> (reward f64 [n],
    done i32 [n])."""
    n = int(_c(state, torch.float64).shape[0])
    for t, dt in ((state, torch.float64), (counter, torch.int64), (ep_steps, torch.int32), (ep_return, torch.float64),
                  (seed, torch.int64), (action, torch.int64)):
        if _dev(t).dtype != dt or not t.is_contiguous() or t.numel() != n * (4 if t is state else 1):
            raise DraError("cartpole_step: contiguous state f64 [n, 4], counter i64, ep_steps i32, ep_return f64, seed i64, action i64 [n]")
    reward = torch.empty(n, dtype=torch.float64, device=state.device)
    done = torch.empty(n, dtype=torch.int32, device=state.device)
    lib.dra_cartpole_step(ptr(state), ptr(counter), ptr(ep_steps), ptr(ep_return), ptr(seed), ptr(action), n, int(horizon),
                          ptr(reward), ptr(done), stream_ptr())
    return reward, done


def categorical_bwd(logits, action, g_lp, g_ent):
    logits = _c(logits, _f32)
    b, a = logits.shape
    out = torch.empty_like(logits)
    lib.dra_categorical_bwd(ptr(logits), b, a, ptr(_c(action, torch.int64)), ptr(None if g_lp is None else _c(g_lp, _f32)),
                            ptr(None if g_ent is None else _c(g_ent, _f32)), ptr(out), stream_ptr())
    return out


def adam_step_counter(param, grad, exp_avg, exp_avg_sq, partials, n_partials, max_norm, lr, beta1, beta2, eps, step_dev,
                      out_norm=None, param_copy=None):
    """Adam whose 1-based step count is the int64 device tensor `step_dev` (bumped by the caller's graph); optional
    mirror of the updated parameters."""
    lib.dra_adam_step_counter(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), ptr(partials),
                              int(n_partials), float(max_norm if max_norm else 0.0), float(lr), float(beta1), float(beta2),
                              float(eps), ptr(step_dev), ptr(out_norm), ptr(param_copy), stream_ptr())


def copy_f32(dst, src):
    lib.dra_copy_f32(ptr(dst), ptr(src), src.numel(), stream_ptr())


def soft_update(target_flat, src_flat, mix):
    """target <- target * (1 - mix) + src * mix over two flat fp32 buffers of equal length (DDPG_agent.py:26-30): one
    launch of `dra_soft_update`; both products are rounded to fp32 before the add, as in the reference's expression."""
    _dev(target_flat), _dev(src_flat)
    if target_flat.numel() != src_flat.numel() or target_flat.dtype != torch.float32 or src_flat.dtype != torch.float32:
        raise DraError("soft_update: two float32 buffers of equal length")
    keep = float(np.float32(1.0 - mix))
    lib.dra_soft_update(ptr(target_flat), ptr(src_flat), target_flat.numel(), keep, float(mix), stream_ptr())
