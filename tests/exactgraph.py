"""Host side of the exact checks of the autograd plumbing (tests/test_graph_exact_cpu.py, tests/test_graph_exact_gpu.py).  No GPU is touched on import.

dcvgan_amd/ops.py decides per call, from mutable state, which entry point runs and which gradient autograd is handed as None because it was already added somewhere
(GradSlot, act_applied, grad_target / note_first / deliver_small, the pack cache, the companion stream, fan_out).  The kernels are held bit for bit by the other exact
suites; here small GRAPHS are built twice from one description — once through a `Device` backend (ops.*) and once through a `Host` backend (torch.nn.functional, fp64,
CPU, ordinary autograd, no project code) — and run through the same call pattern (one backward, retain_graph twice, a pruned autograd.grad first, ...).

Operands are integer-valued (activations and cotangents in [-3, 3], weights in {-1, 0, 1} with a seeded sparsity, LeakyReLU slope 1/4 or 0, hinge losses over a power
of two of logits), so every forward value and every gradient is an fp32 number and any order of adding the partial products is exact.  The twin PROVES that per case
(`prove`): a third build with every operand replaced by its magnitude and every activation by the identity bounds each partial sum of the real graph; on the grid of the
products (`grid_of`) that bound must stay below 2^24, and each expected tensor must survive a round trip through fp32.  A case that claims exactness it does not have
fails on the host.

`Recorder` is the recording proxy for the library handle: installed over the module-level name `lib` of ops / ops_cl, it forwards every call and notes the entry point
(and a DCV_EUNSUPPORTED refusal), so that every case can state the multiset of launches it expects — a route that silently falls back then fails its case."""
import contextlib
import zlib
from collections import Counter, OrderedDict

import torch
import torch.nn.functional as F

SLOPES = (0.25, 0.0)
KIND_HINGE_REAL, KIND_HINGE_FAKE = 2, 3                 # ops.KIND_HINGE_REAL / ops.KIND_HINGE_FAKE (test_graph_exact_cpu.py pins them)
EUNSUPPORTED = -4                                       # native.DCV_EUNSUPPORTED
# entry points that launch nothing (sizes, capabilities, the error text): not part of a case's multiset
QUERIES = ("dcv_conv_workspace_bytes", "dcv_conv_packed_bytes", "dcv_conv_effective_precision", "dcv_conv_stats_bytes", "dcv_bn_workspace_bytes",
           "dcv_gru_workspace_bytes", "dcv_last_error", "dcv_conv_backward_data_bn_workspace_bytes", "dcv_launch_count", "dcv_debug_last_kernel")


def seed_of(name):
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the recording proxy
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands where `lib` stands (`lib()` returns the handle): `Recorder(real_handle)()` is the recorder itself, every attribute a forwarding wrapper."""

    def __init__(self, real):
        self._real = real
        self.calls = []          # names in call order; "<name>!refused" when the entry point returned DCV_EUNSUPPORTED

    def __call__(self):
        return self

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn

        def call(*a, **k):
            rc = fn(*a, **k)
            self.calls.append(name + ("!refused" if (isinstance(rc, int) and not isinstance(rc, bool) and rc == EUNSUPPORTED and name not in QUERIES) else ""))
            return rc
        return call

    def reset(self):
        del self.calls[:]

    def launches(self):
        """The multiset of dcv_* entry points called since the last reset, the queries left out"""
        return Counter(n for n in self.calls if n.startswith("dcv_") and n.split("!")[0] not in QUERIES)


@contextlib.contextmanager
def recording(modules, real):
    """Install one Recorder over the name `lib` of every module in `modules`; restore on exit."""
    rec = Recorder(real)
    saved = [(m, m.lib) for m in modules]
    for m in modules:
        m.lib = rec
    try:
        yield rec
    finally:
        for m, v in saved:
            m.lib = v


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def ints(g, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def ternary(g, shape, density):
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return sign * (torch.rand(tuple(shape), generator=g) < density).double()


def is_f32(t):
    return bool((t.float().double() == t).all())


def grid_of(t):
    """The largest power of two (at most 1) that divides every element of `t`"""
    g = 1.0
    while not bool(((t / g) == (t / g).round()).all()):
        g /= 2
        assert g > 2.0 ** -60, "not on a binary grid"
    return g


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the two backends.  A description calls only these methods.
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class Host:
    """fp64 on the CPU, torch.nn.functional under ordinary autograd.  `magnitude`: the bounding build — operands are magnitudes, activations the identity, differences
    sums, the hinge's derivative 1/n everywhere: every value of that build bounds the sum of the magnitudes of the terms of its counterpart."""
    device = torch.device("cpu")

    def __init__(self, magnitude=False, exact=True):
        self.magnitude, self.exact = magnitude, exact      # exact=False: real-valued operands (gradcheck): no claim is checked
        self.nodes = []          # per convolution: dict(x, w, y, dys=[...]) in call order

    def leaf(self, v, kind):
        v = v.abs() if self.magnitude else v
        t = v.clone().double()
        return t.requires_grad_(True) if kind != "const" else t

    def value(self, t):
        return None if t is None else t.detach().clone()

    def buffer(self, n, ca, cb, spatial):
        return None

    def conv(self, x, w, stride, padding, transposed=False, act=None, out=None, grad_slot=None, act_slot=None, gate=None):
        if transposed:
            y = F.conv_transpose2d(x, w, None, stride, padding)
        else:
            y = (F.conv2d if w.dim() == 4 else F.conv3d)(x, w, None, stride, padding)
        node = dict(x=x, w=w, y=y, dys=[], douts=[])
        self.nodes.append(node)
        if y.requires_grad:
            y.register_hook(lambda g, node=node: None if g is None else node["dys"].append(g.detach().clone()))
            if x.requires_grad:
                x.retain_grad()
        if act is not None:
            y = y * 1.0 if self.magnitude else F.leaky_relu(y, act)      # (a tensor of its own in either build: hooks on the two must not meet)
            if y.requires_grad:
                y.register_hook(lambda g, node=node: None if g is None else node["douts"].append(g.detach().clone()))
        node["out"] = y
        return y

    def bn_act(self, x, gamma, beta, act=None, out=None, eps=0.0):
        y = F.batch_norm(x, None, None, gamma, beta, True, 0.0, eps)
        return y if act is None else F.leaky_relu(y, act)

    def join(self, buf, a, b):
        return torch.cat([a, b], 1)

    def noise(self, x, sample):
        return x + (sample.abs() if self.magnitude else sample)

    def cat_channels(self, a, b):
        return torch.cat([a, b], 1)

    def copy_into(self, x, buf, which):
        return x + 0

    def temporal_diff(self, x):
        return x[:, :, 1:] + x[:, :, :-1] if self.magnitude else x[:, :, 1:] - x[:, :, :-1]

    def fan_out(self, x, t, n_full):
        return (x[:, :, t],) + tuple(x for _ in range(n_full))

    def segm_onehot(self, x):
        """ops.segm_onehot: {-1, +1} maps by channel arg-max, the FIRST maximum on a tie; no gradient passes"""
        with torch.no_grad():
            y = torch.full_like(x, -1.0).scatter_(1, x.argmax(1, keepdim=True), 1.0)
            return y.abs() if self.magnitude else y

    def fan_geometry(self, x, t, rows):
        """augment.ClipAugment.fan_geometry under a fixed table of flips, shifts and cutouts (the geometry stream moves values, tests/test_augment_cpu.py::forward_ref),
        in fan_out's order: (frame t of the augmented clip, x itself for the colour generator, the augmented clip twice)"""
        H, W = x.shape[3], x.shape[4]
        hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        planes = []
        for b, r in enumerate(rows):
            cy0, cx0, cs = r.get("cy0", 0), r.get("cx0", 0), r.get("cs", 0)
            cut = (hh >= cy0) & (hh < cy0 + cs) & (ww >= cx0) & (ww < cx0 + cs)
            hs, ws = hh - r.get("dy", 0), ww - r.get("dx", 0)
            ok = ~cut & (hs >= 0) & (hs < H) & (ws >= 0) & (ws < W)
            wsrc = W - 1 - ws if r.get("flip", 0) else ws
            planes.append(x[b][:, :, hs.clamp(0, H - 1), wsrc.clamp(0, W - 1)] * ok.to(x.dtype))
        y = torch.stack(planes)
        return y[:, :, t], x, y, y

    def hinge_sum(self, terms):
        tot = None
        for y, kind in terms:
            if self.magnitude:
                v = (1.0 + y).mean()
            else:
                v = F.relu(1.0 - y).mean() if kind == KIND_HINGE_REAL else F.relu(1.0 + y).mean()
                assert not self.exact or is_f32(v.detach()), "a hinge term's value is not an fp32 number"      # (dcv_gan_loss sums in fp64 and rounds once, tests/exactew.py)
            tot = v if tot is None else tot + v
        return tot

    def sum_scalars(self, *xs):
        tot = xs[0]
        for x in xs[1:]:
            tot = tot + x
        return tot

    def gru(self, e, h0, w_ih, w_hh, b_ih, b_hh):
        dm = e.shape[2]
        h, outs = h0, []
        for t in range(e.shape[0]):
            gi, gh = e[t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
            r = torch.sigmoid(gi[:, :dm] + gh[:, :dm])
            z = torch.sigmoid(gi[:, dm:2 * dm] + gh[:, dm:2 * dm])
            n = torch.tanh(gi[:, 2 * dm:] + r * gh[:, 2 * dm:])
            h = n + z * (h - n)
            outs.append(h)
        return torch.stack(outs, 1)

    def cot(self, v):
        return (v.abs() if self.magnitude else v).clone().double()

    def out(self, y):
        return y


class Device:
    """dcvgan_amd.ops on the GPU.  Weights are nn.Parameters (the accumulation routes are keyed on that), inputs plain leaves."""

    def __init__(self, device):
        from dcvgan_amd import ops
        self.ops, self.device = ops, device
        self.buffers = []

    def leaf(self, v, kind):
        t = v.float().to(self.device)
        if kind == "param":
            return torch.nn.Parameter(t)
        return t.requires_grad_(True) if kind == "input" else t

    def value(self, t):
        return None if t is None else t.detach().cpu().clone()

    def buffer(self, n, ca, cb, spatial):
        b = self.ops.ConcatBuffer(n, ca, cb, tuple(spatial), self.device)
        self.buffers.append(b)
        return b

    def conv(self, x, w, stride, padding, transposed=False, act=None, out=None, grad_slot=None, act_slot=None, gate=None):
        o = self.ops
        dst = None if out is None else (out[0].first if out[1] == "first" else out[0].second)
        return o.conv(x, w, o.conv_geom(w, stride, padding, transposed), o.ACT_NONE if act is None else o.ACT_LEAKY, 0.0 if act is None else act, out=dst,
                      grad_slot=None if grad_slot is None else grad_slot.slot, act_slot=None if act_slot is None else act_slot.slot,
                      gate=None if gate is None else (gate.buf, gate.slot))

    def bn_act(self, x, gamma, beta, act=None, out=None, eps=0.0):
        o = self.ops
        dst = None if out is None else (out[0].first if out[1] == "first" else out[0].second)
        return o.bn_act(x, gamma, beta, None, None, True, o.ACT_NONE if act is None else o.ACT_LEAKY, 0.0 if act is None else act, eps=eps, out=dst)

    def join(self, buf, a, b):
        return buf.join(a, b)

    def noise(self, x, sample):
        return self.ops.noise_add(x, 1.0, sample=sample)

    def cat_channels(self, a, b):
        return self.ops.cat_channels(a, b)

    def copy_into(self, x, buf, which):
        return self.ops.copy_into(x, buf.first if which == "first" else buf.second)

    def temporal_diff(self, x):
        return self.ops.temporal_diff(x)

    def fan_out(self, x, t, n_full):
        return self.ops.fan_out(x, t, n_full)

    def segm_onehot(self, x):
        return self.ops.segm_onehot(x)

    def fan_geometry(self, x, t, rows):
        from types import SimpleNamespace
        from dcvgan_amd import augment
        from tests.test_augment_cpu import make_table
        aug = augment.ClipAugment(SimpleNamespace(batchsize=x.shape[0], geometric_info="segmentation"), self.device, p=1.0, adaptive=False)
        g_c, g_i, g_v, g_g = aug.fan_geometry(x, t, torch.from_numpy(make_table(rows)).to(self.device))
        return g_i, g_c, g_v, g_g

    def hinge_sum(self, terms):
        return self.ops.gan_loss_sum(list(terms))

    def sum_scalars(self, *xs):
        return self.ops.sum_scalars(*xs)

    def gru(self, e, h0, w_ih, w_hh, b_ih, b_hh):
        return self.ops.gru_sequence(e, h0, w_ih, w_hh, b_ih, b_hh)

    def cot(self, v):
        return v.float().to(self.device)

    def out(self, y):
        return y


class DeviceLayers(Device):
    """As Device, every convolution (+ activation) as an nn.Sequential of torch modules holding the SAME Parameter, executed by dcvgan_amd.layers.run: what run adds
    (grouping conv + activation, passing out= / grad_slot= / act_slot= / gate= to the first or last fused op) must change neither a launch nor a word."""

    def conv(self, x, w, stride, padding, transposed=False, act=None, out=None, grad_slot=None, act_slot=None, gate=None):
        from dcvgan_amd import layers
        nn = torch.nn
        cls = nn.ConvTranspose2d if transposed else (nn.Conv2d if w.dim() == 4 else nn.Conv3d)
        a, b = w.shape[0], w.shape[1]
        m = cls(a if transposed else b, b if transposed else a, tuple(w.shape[2:]), tuple(stride), tuple(padding), bias=False)
        m.weight = w
        seq = nn.Sequential(*([m] + ([nn.LeakyReLU(act) if act else nn.ReLU()] if act is not None else [])))
        dst = None if out is None else (out[0].first if out[1] == "first" else out[0].second)
        return layers.run(seq, x, None, out=dst, grad_slot=None if grad_slot is None else grad_slot.slot, act_slot=None if act_slot is None else act_slot.slot,
                          gate=None if gate is None else (gate.buf, gate.slot))


class DeviceCL(Device):
    """The 16-bit channels-last path: fp32 leaves enter through ops_cl.from_f32, the convolutions, the concat buffer and its slot are ops_cl's own, the output leaves
    through ops_cl.to_f32.  The element type is whatever ops_cl._HALF holds (the tests patch it).  No gate=: ops_cl has no stem gate."""

    def __init__(self, device):
        super().__init__(device)
        from dcvgan_amd import ops_cl
        self.cl = ops_cl

    def buffer(self, n, ca, cb, spatial):
        b = self.cl.ConcatBuffer(n, ca, cb, tuple(spatial), self.device)
        self.buffers.append(b)
        return b

    def conv(self, x, w, stride, padding, transposed=False, act=None, out=None, grad_slot=None, act_slot=None, gate=None):
        assert gate is None
        o, cl = self.ops, self.cl
        if not cl.is_cl(x):
            x = cl.from_f32(x)
        dst = None if out is None else (out[0].first if out[1] == "first" else out[0].second)
        return cl.conv(x, w, o.conv_geom(w, stride, padding, transposed), o.ACT_NONE if act is None else o.ACT_LEAKY, 0.0 if act is None else act, out=dst,
                       grad_slot=None if grad_slot is None else grad_slot.slot, act_slot=None if act_slot is None else act_slot.slot)

    def out(self, y):
        return self.cl.to_f32(y)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the graphs.  spec: name -> (shape, kind, generator) with kind "param" | "input" | "const"; fn(B, L) -> (outputs, taps)
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class Graph:
    """One description.  `fwd` / `bwd`: the launches of one forward / of one full backward whose parameter gradients are FIRST contributions; `late`: (parameter,
    launches) of torch.autograd.grad towards that parameter alone.  `small`: parameters delivered through deliver_small."""

    def __init__(self, name, spec, fn, fwd, bwd, late, cots, shapes, small=()):
        self.name, self.spec, self.fn, self.fwd, self.bwd, self.late, self.cots, self.shapes, self.small = name, spec, fn, Counter(fwd), Counter(bwd), late, cots, shapes, small

    def values(self, tag=""):
        g = torch.Generator().manual_seed(seed_of(self.name + tag))
        out = OrderedDict()
        for n, (shape, kind, gen) in self.spec.items():
            v = gen(g, shape)
            out[n] = v
        return out

    def kinds(self):
        return {n: k for n, (_, k, _) in self.spec.items()}

    def leaves(self, B, frozen=(), tag="", share=None):
        """`share`: leaves of an earlier build whose parameters this one reuses (the same modules on another batch)"""
        L = OrderedDict()
        for n, v in self.values(tag).items():
            kind = self.kinds()[n]
            if share is not None and kind == "param":
                L[n] = share[n]
            else:
                L[n] = B.leaf(v, "const" if (n in frozen or kind in frozen) else kind)
        return L

    def cotangents(self, B, tag=""):
        g = torch.Generator().manual_seed(seed_of(self.name + ":cot" + tag))
        return [B.cot(ints(g, s)) for s in self.cots]

    def later(self, c, own=True):
        """The launches of a backward whose parameter gradients are LATER contributions (a .grad exists, or the second use in one backward)"""
        c = Counter(c)
        if own:
            n = c.pop("dcv_conv_backward_weight", 0)
            if n:
                c["dcv_conv_backward_weight_acc"] += n
            if self.small:
                c["dcv_axpby"] += len(self.small) * max(1, c.get("dcv_bn_act_backward", 0) + c.get("dcv_gru_backward", 0))
        return c


def _w(density):
    return lambda g, s: ternary(g, s, density)


def unet_graph(slope, thin=False):
    """conv3s1p1(8 -> cs) + act into the SECOND slice (act_slot); conv4s2p1(cs -> 16) + act reads it (grad_slot); convT4s2p1(16 -> 8) into the first; join;
    conv3s1p1(8 + cs -> 8).  cs = 8, or 4 for the consumer the gated entry refuses."""
    cs = 4 if thin else 8
    spec = OrderedDict(x=((2, 8, 8, 8), "input", ints), w1=((cs, 8, 3, 3), "param", _w(0.15)), w2=((16, cs, 4, 4), "param", _w(0.1)),
                       w3=((16, 8, 4, 4), "param", _w(0.1)), w4=((8, 8 + cs, 3, 3), "param", _w(0.1)))

    def fn(B, L):
        buf = B.buffer(2, 8, cs, (8, 8))
        a = B.conv(L["x"], L["w1"], (1, 1), (1, 1), act=slope, out=(buf, "second"), act_slot=buf)
        d = B.conv(a, L["w2"], (2, 2), (1, 1), act=slope, grad_slot=buf)
        u = B.conv(d, L["w3"], (2, 2), (1, 1), transposed=True, out=(buf, "first"))
        y = B.out(B.conv(B.join(buf, u, a), L["w4"], (1, 1), (1, 1)))
        return [y], dict(skip=a, buf=buf)

    fwd = {"dcv_conv_forward": 4}
    if thin:
        bwd = {"dcv_act_backward": 2, "dcv_conv_backward_data_gated!refused": 1, "dcv_conv_backward_data": 4, "dcv_conv_backward_weight": 4}
    else:
        bwd = {"dcv_act_backward": 1, "dcv_conv_backward_data_gated": 1, "dcv_conv_backward_data": 3, "dcv_conv_backward_weight": 4}
    late = ("w4", {"dcv_conv_backward_data": 1, "dcv_conv_backward_weight": 1})
    return Graph(f"unet{'_thin' if thin else ''}_s{slope}", spec, fn, fwd, bwd, late, [(2, 8, 8, 8)],
                 dict(x=(2, 8, 8, 8), skip=(2, cs, 8, 8), down=(2, 16, 4, 4), buffer=(2, 8 + cs, 8, 8), y=(2, 8, 8, 8)))


def unet_bn_graph():
    """The U-Net stage with a training-mode BatchNorm + ReLU group on the up path, written with out= into the first slice (eps 1e-5).  Behind a convolution the batch
    statistics are no integers: this graph is BOUNDED, not exact (tests/test_graph_exact_gpu.py::test_unet_bn_*), and is kept out of GRAPHS."""
    spec = OrderedDict(x=((2, 8, 8, 8), "input", ints), w1=((8, 8, 3, 3), "param", _w(0.15)), w2=((16, 8, 4, 4), "param", _w(0.1)),
                       w3=((16, 8, 4, 4), "param", _w(0.1)), w4=((8, 16, 3, 3), "param", _w(0.1)),
                       gamma=((8,), "param", lambda g, s: 2.0 ** torch.randint(-1, 2, tuple(s), generator=g).double()), beta=((8,), "param", lambda g, s: ints(g, s, -2, 2)))

    def fn(B, L):
        buf = B.buffer(2, 8, 8, (8, 8))
        a = B.conv(L["x"], L["w1"], (1, 1), (1, 1), act=0.25, out=(buf, "second"), act_slot=buf)
        d = B.conv(a, L["w2"], (2, 2), (1, 1), act=0.25, grad_slot=buf)
        u = B.conv(d, L["w3"], (2, 2), (1, 1), transposed=True)
        b = B.bn_act(u, L["gamma"], L["beta"], act=0.0, out=(buf, "first"), eps=1e-5)
        y = B.conv(B.join(buf, b, a), L["w4"], (1, 1), (1, 1))
        return [y], dict(skip=a, buf=buf, bn_in=u, bn_out=b)

    fwd = {"dcv_conv_forward": 4, "dcv_bn_act_forward": 1}
    bwd = {"dcv_act_backward": 1, "dcv_conv_backward_data_gated": 1, "dcv_conv_backward_data": 3, "dcv_conv_backward_weight": 4, "dcv_bn_act_backward": 1}
    return Graph("unet_bn", spec, fn, fwd, bwd, ("w4", {"dcv_conv_backward_data": 1, "dcv_conv_backward_weight": 1}), [(2, 8, 8, 8)],
                 dict(x=(2, 8, 8, 8), skip=(2, 8, 8, 8), down=(2, 16, 4, 4), buffer=(2, 16, 8, 8), y=(2, 8, 8, 8)), small=("gamma", "beta"))


def dfront_graph(slope, three_d=False):
    """Two conv4s2p1(8 -> 8) + act stems into the halves of one buffer (act_slot), join, a Noise copy with an injected integer sample, conv4s2p1(16 -> 16) with gate=."""
    if three_d:
        k, s, p, sp_in, sp_mid, sp_out = (4, 4, 4), (1, 2, 2), (0, 1, 1), (7, 8, 8), (4, 4, 4), (1, 2, 2)
    else:
        k, s, p, sp_in, sp_mid, sp_out = (4, 4), (2, 2), (1, 1), (16, 16), (8, 8), (4, 4)
    spec = OrderedDict(xg=((2, 8) + sp_in, "input", ints), xc=((2, 8) + sp_in, "input", ints), wg=((8, 8) + k, "param", _w(0.1 if three_d else 0.2)),
                       wc=((8, 8) + k, "param", _w(0.1 if three_d else 0.2)), wm=((16, 16) + k, "param", _w(0.05 if three_d else 0.1)),
                       sample=((2, 16) + sp_mid, "const", ints))

    def fn(B, L):
        buf = B.buffer(2, 8, 8, sp_mid)
        hg = B.conv(L["xg"], L["wg"], s, p, act=slope, out=(buf, "second"), act_slot=buf)
        hc = B.conv(L["xc"], L["wc"], s, p, act=slope, out=(buf, "first"), act_slot=buf)
        h = B.noise(B.join(buf, hc, hg), L["sample"])
        y = B.conv(h, L["wm"], s, p, gate=buf)
        return [y], dict(skip=hg, first=hc, buf=buf)

    fwd = {"dcv_conv_forward": 3, "dcv_axpby": 1}
    bwd = {"dcv_conv_backward_data_gated": 1, "dcv_conv_backward_data": 2, "dcv_conv_backward_weight": 3}
    late = ("wm", {"dcv_conv_backward_data_gated": 1, "dcv_conv_backward_weight": 1})
    return Graph(f"dfront{'3d' if three_d else ''}_s{slope}", spec, fn, fwd, bwd, late, [(2, 16) + sp_out],
                 dict(x=(2, 8) + sp_in, buffer=(2, 16) + sp_mid, y=(2, 16) + sp_out))


SEGM_AUG_ROWS = (dict(flip=1, dx=1, dy=-1, cy0=1, cx0=2, cs=3), dict(dx=-2, dy=1, cy0=5, cx0=-1, cs=4))      # one row per clip: every branch of the geometry stream


def segmfront_graph(slope, augmented=False):
    """The generators' front of the segmentation iteration (trainer.StepRunner._colour): a (B, T, C, H, W) clip of C = 25 maps viewed as (B, C, T, H, W), fanned out
    to four readers — frame t through conv4s2p1(25 -> 8) + act (the image discriminator's geometry stem), the clip through conv3d (4,4,4) s(1,2,2)(25 -> 8) + act
    (the video discriminator's), its temporal difference through another (the gradient discriminator's), and the colour generator: the frames through segm_onehot
    (no gradient passes) into the U-Net stage of unet_graph, whose stem conv3s1p1(25 -> 8) + act has NO data gradient while its act_slot is armed.  The clip's ONE
    gradient is formed from three cotangents and a None.  `augmented`: augment.fan_geometry under SEGM_AUG_ROWS in fan_out's place (_AugFan has the same branch)."""
    Bn, T, Cg, S, t = 2, 5, 25, 8, 2
    spec = OrderedDict(x=((Bn, T, Cg, S, S), "input", ints), w1=((8, Cg, 3, 3), "param", _w(0.04)), w2=((16, 8, 4, 4), "param", _w(0.1)),
                       w3=((16, 8, 4, 4), "param", _w(0.1)), w4=((8, 16, 3, 3), "param", _w(0.1)), wi=((8, Cg, 4, 4), "param", _w(0.1)),
                       wv=((8, Cg, 4, 4, 4), "param", _w(0.05)), wg=((8, Cg, 4, 4, 4), "param", _w(0.05)))

    def fn(B, L):
        clip = L["x"].permute(0, 2, 1, 3, 4)                                  # the generators' layout: a view
        g_i, g_c, g_v, g_g = B.fan_geometry(clip, t, SEGM_AUG_ROWS) if augmented else B.fan_out(clip, t, 3)
        maps = B.segm_onehot(g_c.permute(0, 2, 1, 3, 4).reshape(Bn * T, Cg, S, S))      # forward_videos' frames: a view again
        buf = B.buffer(Bn * T, 8, 8, (S, S))
        a = B.conv(maps, L["w1"], (1, 1), (1, 1), act=slope, out=(buf, "second"), act_slot=buf)
        d = B.conv(a, L["w2"], (2, 2), (1, 1), act=slope, grad_slot=buf)
        u = B.conv(d, L["w3"], (2, 2), (1, 1), transposed=True, out=(buf, "first"))
        yc = B.out(B.conv(B.join(buf, u, a), L["w4"], (1, 1), (1, 1)))
        yi = B.conv(g_i, L["wi"], (2, 2), (1, 1), act=slope)
        yv = B.conv(g_v, L["wv"], (1, 2, 2), (0, 1, 1), act=slope)
        yg = B.conv(B.temporal_diff(g_g), L["wg"], (1, 2, 2), (0, 1, 1), act=slope)
        return [yc, yi, yv, yg], dict(skip=a, buf=buf, maps=maps)

    fwd = {"dcv_segm_onehot": 1, "dcv_conv_forward": 7, "dcv_axpby": 1}
    # seven weight gradients and SIX data gradients: none for the stem.  dcv_axpby: three of temporal_diff's backward, two of fan_out's (vdis + gdis, then the frame)
    bwd = {"dcv_act_backward": 4, "dcv_conv_backward_data_gated": 1, "dcv_conv_backward_data": 5, "dcv_conv_backward_weight": 7, "dcv_axpby": 5}
    if augmented:
        fwd["dcv_aug_apply"] = 1
        bwd.update({"dcv_axpby": 3, "dcv_aug_fan_backward": 1})
    late = ("w4", {"dcv_conv_backward_data": 1, "dcv_conv_backward_weight": 1})
    return Graph(f"segmfront{'_aug' if augmented else ''}_s{slope}", spec, fn, fwd, bwd, late,
                 [(Bn * T, 8, S, S), (Bn, 8, S // 2, S // 2), (Bn, 8, T - 3, S // 2, S // 2), (Bn, 8, T - 4, S // 2, S // 2)],
                 dict(x=(Bn, T, Cg, S, S), maps=(Bn * T, Cg, S, S), skip=(Bn * T, 8, S, S), buffer=(Bn * T, 16, S, S), y=(Bn * T, 8, S, S)))


def psum_graph(slope):
    """One weight, conv4s2p1(8 -> 8) + act; the call patterns run it on two batches (real and fake)"""
    spec = OrderedDict(x=((2, 8, 8, 8), "input", ints), w=((8, 8, 4, 4), "param", _w(0.25)))

    def fn(B, L):
        y = B.out(B.conv(L["x"], L["w"], (2, 2), (1, 1), act=slope))
        return [y], dict(skip=y)

    return Graph(f"psum_s{slope}", spec, fn, {"dcv_conv_forward": 1}, {"dcv_act_backward": 1, "dcv_conv_backward_data": 1, "dcv_conv_backward_weight": 1},
                 ("w", {"dcv_act_backward": 1, "dcv_conv_backward_data": 1, "dcv_conv_backward_weight": 1}), [(2, 8, 4, 4)], dict(x=(2, 8, 8, 8), y=(2, 8, 4, 4)))


def unet_cl_graph():
    """The U-Net stage in a value range the 16-bit formats hold exactly: inputs in [-1, 1], sparser weights (every stored tensor: 8 significant bits, |v| <= 256)"""
    g = unet_graph(0.0)      # ReLU: everything stays an integer (slope 1/4 twice costs four of the eight bits)
    d = {"w1": 0.08, "w2": 0.05, "w3": 0.06, "w4": 0.05}
    g.name = "unet_cl"
    g.spec = OrderedDict((n, (sh, k, (lambda gen, s: ints(gen, s, -1, 1)) if n == "x" else _w(d[n]))) for n, (sh, k, _) in g.spec.items())
    return g


def psum_cl_graph():
    g = psum_graph(0.25)
    g.name = "psum_cl"
    return g


def is_half_exact(t):
    """bf16 and fp16 both hold `t` exactly, |t| <= 256"""
    return bool(((t.bfloat16().double() == t) & (t.half().double() == t) & (t.abs() <= 256)).all())


def prove_cl(graph, pattern, cot_hi=1):
    """As prove, and every tensor the 16-bit path STORES (a convolution's input, its output after the activation, both cotangents, the data gradient with what is
    accumulated into it, the loss's gradient) is a bf16 and an fp16 value below 256 in magnitude: the path's results are then the twin's words, the fp32 weight
    gradients included (fp32 accumulation of exact products, as on the fp32 path)."""
    H = Host()
    res, _ = run_pattern(H, graph, pattern)
    for i, a in enumerate(H.nodes):
        stored = [("input", a["x"].detach()), ("output", a["out"].detach())] + [("dz", d) for d in a["dys"]] + [("dy", d) for d in a["douts"]]
        if a["x"].grad is not None:
            stored.append(("dx", a["x"].grad))
        for what, t in stored:
            assert is_half_exact(t), f"{graph.name} {pattern}: convolution {i} {what} is not held by the 16-bit formats (max {float(t.abs().max())})"
    return prove(graph, pattern)[0]


GRAPHS = OrderedDict((g.name, g) for g in (
    [unet_graph(s) for s in SLOPES] + [unet_graph(0.25, thin=True)] + [dfront_graph(s) for s in SLOPES] + [dfront_graph(0.25, three_d=True)]
    + [psum_graph(s) for s in SLOPES] + [segmfront_graph(0.25)]))
PATTERN_GRAPHS = ("unet_s0.25", "dfront_s0.25", "psum_s0.25")


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the call patterns: the same code runs on either backend -> OrderedDict name -> tensor on the host (None where autograd delivered nothing)
# `rec`: a Recorder or None; `marks`: receives (label, launches since the previous mark)
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class Boom(Exception):
    """The hook's exception of pattern 4: an ordinary Python exception raised on the host"""


def _grads(B, L, res, tag):
    for n, t in L.items():
        if t.requires_grad:
            res[f"{tag}d{n}"] = B.value(t.grad)


def _mark(rec, marks, label):
    if rec is not None:
        marks.append((label, rec.launches()))
        rec.reset()


def run_pattern(B, graph, pattern, rec=None, frozen=()):
    res, marks = OrderedDict(), []
    if rec is not None:
        rec.reset()
    L = graph.leaves(B, frozen)
    cots = graph.cotangents(B)

    def forward(LL, label="fwd"):
        outs, taps = graph.fn(B, LL)
        _mark(rec, marks, label)
        return outs, taps

    if pattern in ("once", "no_input", "no_weight", "neither"):
        outs, _ = forward(L)
        res["y"] = B.value(outs[0])
        if outs[0].requires_grad:
            torch.autograd.backward(outs, cots)
            _mark(rec, marks, "bwd")
        _grads(B, L, res, "")
    elif pattern == "retain_twice":
        outs, _ = forward(L)
        torch.autograd.backward(outs, cots, retain_graph=True)
        _mark(rec, marks, "bwd")
        _grads(B, L, res, "first:")
        torch.autograd.backward(outs, cots, retain_graph=True)
        _mark(rec, marks, "bwd_later")
        _grads(B, L, res, "second:")
    elif pattern == "pruned_first":
        outs, _ = forward(L)
        (g_late,) = torch.autograd.grad(outs, [L[graph.late[0]]], cots, retain_graph=True)
        _mark(rec, marks, "late")
        res["late"] = B.value(g_late)
        torch.autograd.backward(outs, cots, retain_graph=True)
        _mark(rec, marks, "bwd")
        _grads(B, L, res, "full:")
        outs2, _ = forward(L)
        torch.autograd.backward(outs2, cots)
        _mark(rec, marks, "bwd_later")
        _grads(B, L, res, "fresh:")
    elif pattern == "grad_beside_grads":
        # .grad holds an earlier backward's gradients; torch.autograd.grad must return whole gradients and leave .grad alone — towards everything, and towards the
        # inputs alone (the parameters' gradients, used twice, are then dropped by the engine as soon as they are returned: nothing may be added to them later)
        outs, _ = forward(L)
        torch.autograd.backward(outs, cots)
        _mark(rec, marks, "bwd")
        _grads(B, L, res, "before:")
        outs2, _ = forward(L)
        wanted = [t for t in L.values() if t.requires_grad]
        gs = torch.autograd.grad(outs2, wanted, cots)
        _mark(rec, marks, "grad_all")
        for n, g_ in zip([n for n, t in L.items() if t.requires_grad], gs):
            res[f"grad:d{n}"] = B.value(g_)
        _grads(B, L, res, "kept:")
        L2 = graph.leaves(B, frozen, tag=":fake", share=L)
        ya, _ = forward(L)
        yb, _ = forward(L2)
        ins = [(n, LL[n]) for LL in (L, L2) for n in LL if graph.kinds()[n] == "input"]
        gs = torch.autograd.grad(ya + yb, [t for _, t in ins], cots + graph.cotangents(B, ":fake"))
        _mark(rec, marks, "grad_inputs")
        for i, ((n, _), g_) in enumerate(zip(ins, gs)):
            res[f"inputs{i}:d{n}"] = B.value(g_)
        _grads(B, L, res, "kept2:")
    elif pattern == "hook_raises":
        outs, taps = forward(L)

        def hook(g):
            raise Boom("the skip gradient's hook")
        taps["skip"].register_hook(hook)
        try:
            torch.autograd.backward(outs, cots)
            raise AssertionError("the hook did not fire")
        except Boom:
            pass
        for t in L.values():
            t.grad = None
        if rec is not None:
            rec.reset()
        outs2, _ = forward(L)
        res["y"] = B.value(outs2[0])
        torch.autograd.backward(outs2, cots)
        _mark(rec, marks, "bwd")
        _grads(B, L, res, "")
    elif pattern in ("two_forwards_summed", "two_forwards_sequential"):
        L2 = graph.leaves(B, frozen, tag=":fake", share=L)
        ya, _ = forward(L)
        yb, _ = forward(L2)
        if pattern == "two_forwards_summed":
            loss = B.hinge_sum([(ya[0], KIND_HINGE_REAL), (yb[0], KIND_HINGE_FAKE)])
            _mark(rec, marks, "loss2")
            res["loss"] = B.value(loss)
            loss.backward()
            _mark(rec, marks, "bwd_both")
        else:
            la, lb = B.hinge_sum([(ya[0], KIND_HINGE_REAL)]), B.hinge_sum([(yb[0], KIND_HINGE_FAKE)])
            _mark(rec, marks, "loss1+1")
            res["loss_a"], res["loss_b"] = B.value(la), B.value(lb)
            la.backward()
            _mark(rec, marks, "bwd_loss")
            lb.backward()
            _mark(rec, marks, "bwd_loss_later")
        _grads(B, L, res, "")
        _grads(B, OrderedDict((n, t) for n, t in L2.items() if graph.kinds()[n] != "param"), res, "fake:")
    elif pattern == "no_grad_between":
        outs, _ = forward(L)
        with torch.no_grad():
            other, _ = forward(graph.leaves(B, frozen, tag=":fake", share=L), "fwd_no_grad")
        res["y"], res["y_no_grad"] = B.value(outs[0]), B.value(other[0])
        torch.autograd.backward(outs, cots)
        _mark(rec, marks, "bwd")
        _grads(B, L, res, "")
    elif pattern.startswith("cot_"):
        outs, _ = forward(L)
        y = outs[0]
        g = torch.Generator().manual_seed(seed_of(graph.name + pattern))
        if pattern == "cot_expand":                      # y.sum(): autograd hands the node an expanded 0-d value (every stride 0)
            y.sum().backward()
        elif pattern == "cot_permuted":                  # a transposed view of a tensor with the last two dimensions swapped
            shape = list(y.shape)
            shape[-1], shape[-2] = shape[-2], shape[-1]
            c = B.cot(ints(g, shape)).transpose(-1, -2)
            assert not c.is_contiguous() or c.shape[-1] == 1 or c.shape[-2] == 1
            y.backward(c)
        elif pattern == "cot_broadcast":                 # one plane of values expanded over the channels: stride 0 in ONE dimension
            c = B.cot(ints(g, (y.shape[0], 1) + tuple(y.shape[2:]))).expand(*y.shape)
            assert c.stride(1) == 0
            y.backward(c)
        elif pattern == "cot_slice":                     # channels [2, 2 + C) of a wider tensor
            wide = B.cot(ints(g, (y.shape[0], y.shape[1] + 5) + tuple(y.shape[2:])))
            y.backward(wide[:, 2:2 + y.shape[1]])
        else:
            raise ValueError(pattern)
        _mark(rec, marks, "bwd")
        _grads(B, L, res, "")
    else:
        raise ValueError(pattern)
    return res, marks


PATTERNS = ("once", "retain_twice", "pruned_first", "grad_beside_grads", "hook_raises", "two_forwards_summed", "two_forwards_sequential", "no_grad_between",
            "cot_expand", "cot_broadcast", "cot_permuted", "cot_slice", "no_input", "no_weight", "neither")
FROZEN = {"no_input": ("input",), "no_weight": ("param",), "neither": ("input", "param")}
LOSS_LAUNCHES = {"loss2": {"dcv_gan_loss": 2}, "loss1+1": {"dcv_gan_loss": 2}}


def expected_marks(graph, pattern, own=True):
    """The launches the Device build must make, mark by mark, for the patterns whose backward is whole.  (The frozen patterns are asserted by what must be ABSENT:
    see test_graph_exact_gpu.py.)"""
    f, b, bl = graph.fwd, graph.bwd, graph.later(graph.bwd, own)
    scale = Counter({"dcv_scale_dev": 1})
    table = {
        "once": [("fwd", f), ("bwd", b)],
        "retain_twice": [("fwd", f), ("bwd", b), ("bwd_later", bl)],
        "pruned_first": [("fwd", f), ("late", Counter(graph.late[1])), ("bwd", b), ("fwd", f), ("bwd_later", bl)],
        # torch.autograd.grad never ends in .grad: every in-place sum stands down, each contribution comes from the plain entry (and the weight gradients nobody asked
        # for are still computed: the nodes cannot know; they are not ADDED anywhere)
        "grad_beside_grads": [("fwd", f), ("bwd", b), ("fwd", f), ("grad_all", b), ("fwd", f), ("fwd", f), ("grad_inputs", b + b)],
        "hook_raises": [("fwd", f), ("fwd", f), ("bwd", b)],      # (the failed backward's own launches are dropped: where it stops is the engine's business)
        "two_forwards_summed": [("fwd", f), ("fwd", f), ("loss2", Counter(LOSS_LAUNCHES["loss2"])), ("bwd_both", b + bl + scale + scale)],
        "two_forwards_sequential": [("fwd", f), ("fwd", f), ("loss1+1", Counter(LOSS_LAUNCHES["loss1+1"])), ("bwd_loss", b + scale), ("bwd_loss_later", bl + scale)],
        "no_grad_between": [("fwd", f), ("fwd_no_grad", f), ("bwd", b)],
        "cot_expand": [("fwd", f), ("bwd", b)], "cot_broadcast": [("fwd", f), ("bwd", b)], "cot_permuted": [("fwd", f), ("bwd", b)], "cot_slice": [("fwd", f), ("bwd", b)],
    }
    return table.get(pattern)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the proof of exactness
# ------------------------------------------------------------------------------------------------------------------------------------------------------
LIMIT = 2.0 ** 24


def prove(graph, pattern, frozen=()):
    """Run `pattern` on the Host twin and on its magnitude build; assert that every expected tensor is an fp32 value and that, per convolution, the magnitude build's
    value of every sum (forward, data gradient incl. what is accumulated into it, weight gradient incl. later contributions) stays below 2^24 on the grid of its
    products.  -> (the twin's results, the largest bound / 2^24 met)"""
    H, M = Host(), Host(magnitude=True)
    res, _ = run_pattern(H, graph, pattern, frozen=frozen)
    mag, _ = run_pattern(M, graph, pattern, frozen=frozen)
    for n, t in res.items():
        assert t is None or is_f32(t), f"{graph.name} {pattern}: expected {n} is not an fp32 tensor"
    assert len(H.nodes) == len(M.nodes)
    worst = 0.0
    for i, (a, m) in enumerate(zip(H.nodes, M.nodes)):
        gx, gw = grid_of(a["x"].detach()), grid_of(a["w"].detach())
        need = [("forward", float(m["y"].detach().max()), gx * gw)]
        assert len(a["dys"]) == len(m["dys"])
        if a["dys"]:
            gdy = min(grid_of(d) for d in a["dys"])
            if a["x"].grad is not None:      # the whole gradient of x in the magnitude build: this node's data gradient plus whatever else is added to it
                need.append(("data gradient", float(m["x"].grad.max()), min(gdy * gw, grid_of(a["x"].grad))))
            if a["w"].grad is not None:
                need.append(("weight gradient", float(m["w"].grad.max()), min(gdy * gx, grid_of(a["w"].grad))))
        for what, bound, grid in need:
            assert bound / grid < LIMIT, f"{graph.name} {pattern}: convolution {i} {what}: partial sums may reach {bound} on a grid of {grid}: not below 2^24"
            worst = max(worst, bound / grid / LIMIT)
    for n, t in mag.items():                 # what is summed outside a convolution (a loss VALUE is an fp64 sum rounded once: each term and the total are fp32 values)
        if t is not None and res[n] is not None and not n.startswith("loss"):
            assert float(t.max()) / grid_of(res[n]) < LIMIT, f"{graph.name} {pattern}: {n}"
    return res, worst


def mismatch(name, got, want):
    """None if the device tensor `got` (on the host) holds the fp64 `want` value for value (NaN equals nothing), else a description of the first difference"""
    if want is None or got is None:
        return None if (want is None and got is None) else f"{name}: {'no gradient' if got is None else 'a gradient'} where the twin has {'none' if want is None else 'one'}"
    if tuple(got.shape) != tuple(want.shape):
        return f"{name}: shape {tuple(got.shape)} for {tuple(want.shape)}"
    bad = ~(got.double() == want)
    if not bool(bad.any()):
        return None
    flat = int(bad.reshape(-1).nonzero()[0])
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), want.shape)) if want.dim() else ()
    return f"{name}: {int(bad.sum())} of {bad.numel()} words differ; first at {idx}: got {float(got.reshape(-1)[flat])!r}, expected {float(want.reshape(-1)[flat])!r}"


def same_words(a, b):
    """Bit for bit, None equal to None"""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# the case table (tests/golden/graph_cases.json pins it): route -> cases that expect its entry point
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def case_table():
    t = OrderedDict()
    for g in GRAPHS.values():
        t[g.name] = dict(shapes={k: list(v) for k, v in g.shapes.items()}, forward=dict(sorted(g.fwd.items())), backward=dict(sorted(g.bwd.items())),
                         later=dict(sorted(g.later(g.bwd).items())), pruned=[g.late[0], dict(sorted(g.late[1].items()))])
    return t


ROUTES = {      # route -> (entry point that proves it, graphs that expect it)
    "skip accumulate + gated data gradient (GradSlot.g, act_applied)": ("dcv_conv_backward_data_gated", ("unet_s0.25", "unet_s0.0")),
    "skip accumulate, gated entry refused: two-step fallback": ("dcv_conv_backward_data_gated!refused", ("unet_thin_s0.25",)),
    "stem gate (act_applied 2 -> 1 -> 0)": ("dcv_conv_backward_data_gated", ("dfront_s0.25", "dfront_s0.0", "dfront3d_s0.25")),
    "weight gradient, first contribution": ("dcv_conv_backward_weight", ("psum_s0.25", "psum_s0.0")),
    "skip accumulate + gated data gradient behind a stem without a data gradient (segm_onehot under no_grad)": ("dcv_conv_backward_data_gated", ("segmfront_s0.25",)),
    "weight gradient, later contribution (grad_target)": ("dcv_conv_backward_weight_acc", ("psum_s0.25", "psum_s0.0")),
}


if __name__ == "__main__":      # python -m tests.exactgraph: rewrite the pinned case table
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_cases.json")
    with open(path, "w") as fh:
        json.dump(dict(cases=case_table(), routes={k: [v[0], list(v[1])] for k, v in ROUTES.items()}, patterns=list(PATTERNS)), fh, indent=1)
        fh.write("\n")
    print("wrote", path)
