"""NormalizingFlowModel — drop-in for src/models/normalizing_flow_model.py:4-128.

Same constructor, attributes (`flows`, `batch_norms`, `batch_norm_between_layers`) and
state_dict keys. When every layer routes to its gfx950 kernel, forward/inverse run the layers
back to back on the current stream with the per-sample log-det accumulated IN PLACE by the
kernels (accumulate=1), which is exactly the reference's sequential float32
`log_det_jacobian_sum += log_det` (normalizing_flow_model.py:30-65); there are no
intermediate log-det tensors and no Python-side adds.

`log_prob` / `nll` add the fused Gaussian base term and the float64 NLL partial sums
(csrc/nfx_gauss.hip): the log_prob glue the reference's callers write inline
(README.md:113-114, src/utils.py:39-55, plots/_common.py:201-202).
"""
import collections
import math

import torch
import torch.nn as nn

from .. import _lib
from ..distributed import merge_bn_stats, sync_bn_world
from ..flows import autoregressive as _autoregressive
from ..flows import coupling as _coupling
from ..flows import lowrank as _lowrank
from ..flows import spline as _spline
from ..flows.flow import HipFlow, STATS


class NormalizingFlowModel(nn.Module):
    def __init__(self, flows, batch_norm_between_layers=False):
        super().__init__()
        self.batch_norm_between_layers = batch_norm_between_layers
        if self.batch_norm_between_layers:
            data_dim = flows[0].data_dim if hasattr(flows[0], "data_dim") else None
            if data_dim is None:
                raise ValueError("Cannot use batch_norm_between_layers if flows do not have a 'data_dim' attribute.")
            self.batch_norms = nn.ModuleList([nn.BatchNorm1d(data_dim) for _ in range(len(flows))])
        self.flows = nn.ModuleList(flows)
        # Profiling hook: when set to a list, _hip_chain appends (layer name, start, end) HIP
        # events recorded on the launch stream around every layer kernel (bench.py uses it).
        self.layer_events = None

    # -- reference-order chaining ------------------------------------------------------------
    def forward(self, z):
        if self._hip_chain_ok(z):
            return self._hip_chain(z, 1)
        log_det_jacobian_sum = 0
        for i, flow in enumerate(self.flows):
            z, log_det_jacobian = flow(z)
            log_det_jacobian_sum += log_det_jacobian
            if self.batch_norm_between_layers and i < len(self.flows) - 1:
                bn = self.batch_norms[i]
                if _bn_hip_ok(z):
                    if self.training:
                        _bn_update_running_hip(bn, z)
                    z, log_det_jacobian_sum = _FlowBatchNormFn.apply(
                        z, _as_ld(log_det_jacobian_sum, z), bn.weight, bn.bias, bn, 1)
                    continue
                z = self._apply_batch_norm(bn, z)
                log_det_jacobian_sum += self._batch_norm_log_det_jacobian(bn, z)
        return z, log_det_jacobian_sum

    def inverse(self, x):
        if self._hip_chain_ok(x):
            return self._hip_chain(x, -1)
        if not self.batch_norm_between_layers and _lowrank.fused_stack_ok(list(self.flows), x):
            # Planar / Radial / Sylvester layers with fused_backward on, under grad: one launch each way
            return _lowrank.fused_stack_inverse(list(self.flows), x, owner=self)
        log_det_jacobian_sum = 0
        for i, flow in reversed(list(enumerate(self.flows))):
            if self.batch_norm_between_layers and i < len(self.flows) - 1:
                bn = self.batch_norms[i]
                if _bn_hip_ok(x):
                    x, log_det_jacobian_sum = _FlowBatchNormFn.apply(
                        x, _as_ld(log_det_jacobian_sum, x), bn.weight, bn.bias, bn, -1)
                else:
                    x = self._inverse_batch_norm(bn, x)
                    log_det_jacobian_sum -= self._batch_norm_log_det_jacobian(bn, x)
            x, log_det_jacobian = flow.inverse(x)
            log_det_jacobian_sum += log_det_jacobian
        return x, log_det_jacobian_sum

    # -- between-layer BatchNorm (normalizing_flow_model.py:67-128) ----------------------------
    # Composite torch versions (CPU, float64); fp32 ROCm tensors run csrc/nfx_flowbn.hip.
    def _apply_batch_norm(self, bn_layer, x):
        if self.training:
            with torch.no_grad():
                momentum = bn_layer.momentum if bn_layer.momentum is not None else 0.1
                if sync_bn_world() > 1:  # SyncBN: the moments of every rank's shard
                    mean, var = _synced_moments(x)
                else:
                    mean, var = x.mean(dim=0), x.var(dim=0, unbiased=False)
                bn_layer.running_mean.mul_(1 - momentum).add_(momentum * mean)
                bn_layer.running_var.mul_(1 - momentum).add_(momentum * var)
        gamma = bn_layer.weight.view(1, -1)
        beta = bn_layer.bias.view(1, -1)
        mean = bn_layer.running_mean.view(1, -1)
        var = bn_layer.running_var.view(1, -1)
        return (x - mean) / torch.sqrt(var + bn_layer.eps) * gamma + beta

    def _batch_norm_log_det_jacobian(self, bn_layer, x):
        log_det_per_dim = torch.log(torch.abs(bn_layer.weight)) - 0.5 * torch.log(bn_layer.running_var + bn_layer.eps)
        return log_det_per_dim.sum()

    def _inverse_batch_norm(self, bn_layer, y):
        gamma = bn_layer.weight.view(1, -1)
        beta = bn_layer.bias.view(1, -1)
        mean = bn_layer.running_mean.view(1, -1)
        var = bn_layer.running_var.view(1, -1)
        return (y - beta) / gamma * torch.sqrt(var + bn_layer.eps) + mean

    # -- gfx950 chain ----------------------------------------------------------------------
    def _needs_grad(self, x):
        if not torch.is_grad_enabled():
            return False
        return x.requires_grad or any(p.requires_grad for p in self.parameters())

    def _hip_chain_ok(self, x):
        if x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() != 2:
            return False
        if self._needs_grad(x):
            return False  # per-layer autograd Functions handle gradients
        for f in self.flows:
            if not isinstance(f, HipFlow) or f._route(x) != "hip":
                return False
        if self.batch_norm_between_layers and len(self.flows) > 1 and not _bn_hip_ok(x):
            return False
        return True

    def _hip_chain(self, x, direction, logprob=None):
        """Run every layer's kernel back to back. With logprob=(logp, sums, workspace) (an
        inverse chain), the last layer also writes the Gaussian log-density and float64 NLL
        partials in its epilogue when it has a fused variant; `fused` in the return says
        whether it did."""
        x = _lib.dense(x)
        B = x.shape[0]
        ld = torch.empty(B, device=x.device, dtype=torch.float32)
        n = len(self.flows)
        chain = None
        if not self.batch_norm_between_layers:
            chain = next((m for m in (_coupling, _spline, _lowrank) if m.chain_ok(list(self.flows), x)), None)
        if chain is not None:
            # the whole chain in one launch (csrc/nfx_affine_chain.hip / nfx_affine_schain.hip /
            # nfx_spline_schain_kernel.h / nfx_lowrank_kernel.h), the per-layer kernels' roundings
            out = torch.empty_like(x)
            ev = self.layer_events
            if ev is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if chain is _lowrank:  # (no fused log-density: the caller runs nfx_gauss_logprob)
                chain.chain_launch(list(self.flows), x, out, ld, direction, False, owner=self)
            else:
                chain.chain_launch(list(self.flows), x, out, ld, direction, False, logprob)
            if ev is not None:
                e1.record()
                ev.append((_lib.last_kernel(), e0, e1))
            return (out, ld, chain is not _lowrank) if logprob is not None else (out, ld)
        bufs = [torch.empty_like(x), torch.empty_like(x)]
        order = range(n) if direction > 0 else reversed(range(n))
        cur, k, first, fused = x, 0, True, False
        for i in order:
            if direction < 0 and self.batch_norm_between_layers and i < n - 1:
                # (never the first op: the last flow has no BatchNorm, so ld is initialised)
                out = bufs[k] if bufs[k] is not cur else bufs[k ^ 1]
                _bn_launch(self.batch_norms[i], cur, out, ld, -1)
                cur = out
            out = bufs[k]
            if out is cur:
                k ^= 1
                out = bufs[k]
            ev = self.layer_events
            if ev is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if logprob is not None and i == 0 and self.flows[i]._hip_launch_logprob(
                    cur, out, ld, *logprob, accumulate=not first):
                STATS["hip"] += 1
                fused = True
            else:
                self.flows[i]._hip_launch_counted(cur, out, ld, direction, accumulate=not first)
            if ev is not None:
                e1.record()
                ev.append((_lib.last_kernel(), e0, e1))
            first = False
            cur, k = out, k ^ 1
            if direction > 0 and self.batch_norm_between_layers and i < n - 1:
                bn = self.batch_norms[i]
                if self.training:
                    _bn_update_running_hip(bn, cur)
                out = bufs[k] if bufs[k] is not cur else bufs[k ^ 1]
                _bn_launch(bn, cur, out, ld, 1)
                cur = out
        if logprob is not None:
            return cur, ld, fused
        return cur, ld

    # -- log-density -------------------------------------------------------------------------
    def log_prob(self, x, return_sums=False, workspace=None):
        """log p(x) = log N(z; 0, I) + log|det J_inv| per sample, z = inverse(x).

        With return_sums=True also returns a float64 tensor [sum_i log p(x_i), B] on x's device
        (the partial a data-parallel NLL all-reduces). `workspace`: the fused epilogue's float64
        partials + arrival word (a contiguous uint8 tensor of at least nfx_gauss_workspace_bytes(B)
        bytes based at a 16-byte boundary, else ValueError; any content: ABI 3 tags the arrival
        word per launch); by default one cached per (device,
        current stream), so calls on different streams never share one."""
        if self._hip_chain_ok(x) and len(self.flows) > 0:
            B = x.shape[0]
            logp = torch.empty(B, device=x.device, dtype=torch.float32)
            sums = torch.empty(2, device=x.device, dtype=torch.float64)
            ws = check_gauss_workspace(workspace, B, x.device) if workspace is not None else gauss_workspace(B, x.device)
            z, ld, fused = self._hip_chain(x, -1, logprob=(logp, sums, ws))
            if not fused:
                gauss_logprob(z, ld, logp, sums, ws)
            return (logp, sums) if return_sums else logp
        z, ld = self.inverse(x)
        if z.device.type == "cuda" and z.dtype == torch.float32 and z.dim() == 2 and not self._needs_grad(x):
            logp, sums = gauss_logprob(z, ld, ws=workspace)
        elif z.device.type == "cuda" and z.dtype == torch.float32 and z.dim() == 2:
            # training: the same HIP epilogue under autograd, its adjoint in one HIP kernel
            logp, sums = _GaussLogProbFn.apply(z, ld, workspace)
        else:
            d = z.shape[1]
            logp = -0.5 * (d * math.log(2 * math.pi) + z.pow(2).sum(-1)) + ld
            if not return_sums:  # (no host->device scalar copy: the step stays graph-capturable)
                return logp
            sums = torch.stack([logp.detach().double().sum(),
                                torch.tensor(float(z.shape[0]), dtype=torch.float64, device=z.device)])
        return (logp, sums) if return_sums else logp

    # -- sampling with the base draw on the device ---------------------------------------------
    # z ~ N(0, I) comes from the library's own counter-based generator (csrc/nfx_rng.h): the model
    # keeps, per device, `_nfx_rng[device] = (seed, state)` with state a device uint64[2] = [offset,
    # arrival word]. Every draw reads the offset and advances it by one ON THE DEVICE, so eager
    # calls and replays of a captured graph both draw afresh. Calls sharing one model's state must
    # be stream-ordered (two streams drawing at once would read the same offset).
    def sample_fused_ok(self, num_samples, device):
        """True when sample_fused draws INSIDE the first forward kernel: eval-mode CouplingLayers
        (d in {2, 4, 8}, H <= 128, up to 64k samples) or d = 2 SplineCouplingLayers (any batch) as
        one launch for the whole stack, or a stack whose first layer is an
        InverseAutoregressiveFlow of a shape the IAF tile kernel takes (the library says which:
        nfx_made_sample_supported) with the remaining layers launched one by one. No between-layer
        BatchNorm."""
        if self.batch_norm_between_layers:
            return False
        return self._sample_chain(num_samples, device) is not None or self._sample_iaf_ok(num_samples, device)

    def _sample_chain(self, num_samples, device):
        fl = list(self.flows)
        for m in (_coupling, _spline):
            if m.sample_chain_ok(fl, num_samples, device):
                return m
        return None

    def _sample_iaf_ok(self, num_samples, device):
        dev = torch.device(device)
        if self.training or num_samples <= 0 or dev.type != "cuda" or len(self.flows) == 0:
            return False
        f0 = self.flows[0]
        if not isinstance(f0, _autoregressive.InverseAutoregressiveFlow) or not f0._fused_family():
            return False
        if not _lib.lib().nfx_made_sample_supported(f0.dim, f0.conditioner.hidden_dim, _lib.NFX_IAF_FORWARD):
            return False
        return self._sample_forward_ok(dev)

    def _sample_forward_ok(self, dev):
        """Would the no-grad forward of an fp32 [n, d] tensor on `dev` run the HIP chain?"""
        d = getattr(self.flows[0], "data_dim", None) if len(self.flows) else None
        if dev.type != "cuda" or d is None:
            return False
        with torch.no_grad():
            return self._hip_chain_ok(torch.empty(0, d, device=dev))

    def _sampler_state(self, dev):
        st = getattr(self, "_nfx_rng", None)
        if st is None:
            st = self._nfx_rng = {}
        if dev not in st:
            seed = getattr(self, "_nfx_seed", None)  # seed_sampler(seed) before the first draw
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            st[dev] = (seed, torch.zeros(2, dtype=torch.int64, device=dev))
        return st[dev]

    def seed_sampler(self, seed, device=None):
        """Set the seed of this model's sampling generator and put its offset back to 0: the draws
        that follow are a function of (seed, number of draws since) alone. device=None: every
        device the model has drawn on, and every device it draws on later."""
        seed = int(seed) & ((1 << 64) - 1)
        st = getattr(self, "_nfx_rng", None)
        if st is None:
            st = self._nfx_rng = {}
        if device is None:
            self._nfx_seed = seed
        devs = list(st) if device is None else [_cuda_device(device)]
        for dev in devs:
            if dev in st:
                st[dev][1].zero_()
                st[dev] = (seed, st[dev][1])
            else:
                st[dev] = (seed, torch.zeros(2, dtype=torch.int64, device=dev))

    def sample_fused(self, num_samples, device="cuda", out=None):
        """Flow.sample (src/flows/flow/flow.py:40-54) with the N(0, I) base draw fused into the
        sampling forward: z ~ N(0, I) on the device (Philox4x32-10, this model's own generator
        state, seeded from torch's CPU generator on first use or by seed_sampler) and
        x = forward(z). Coupling and spline stacks: ONE launch (nfx_affine_chain_sample /
        nfx_spline_chain_sample). Stacks that start with an IAF layer: the draw in that layer's
        kernel (nfx_made_affine_sample), the remaining layers launched one by one — L launches
        for L layers. Returns (x, log_det, z); x and log_det equal forward(z) bit for bit.
        out=(z, x, ld) writes into caller buffers (GraphedFlow(mode="sample")): contiguous, each
        based at a 16-byte boundary (the kernels write them in place; ValueError otherwise). Calls sharing
        this model's generator state must be stream-ordered."""
        dev = _cuda_device(device)
        if not self.sample_fused_ok(num_samples, dev):
            raise NotImplementedError("sample_fused: no kernel with the draw fused in takes this model / size "
                                      "(sample_on_device draws with the stand-alone kernel)")
        seed, state = self._sampler_state(dev)
        d = self.flows[0].data_dim
        if out is None:
            z = torch.empty(num_samples, d, device=dev)
            x = torch.empty_like(z)
            ld = torch.empty(num_samples, device=dev)
        else:
            z, x, ld = out
            if any(not t.is_contiguous() or t.data_ptr() & 15 for t in out):
                raise ValueError("sample_fused: out = (z, x, ld) must be contiguous, each based at a 16-byte boundary")
        chain = self._sample_chain(num_samples, dev)
        if chain is not None:
            chain.chain_sample(list(self.flows), state, seed, z, x, ld)
            return x, ld, z
        # IAF first: layer i writes x when an even number of layers follow it, else the spare
        # buffer, so the last layer lands in x and no launch reads the buffer it writes
        n = len(self.flows)
        spare = torch.empty_like(x) if n > 1 else None
        f0 = self.flows[0]
        cur = x if (n - 1) % 2 == 0 else spare
        packed = f0._packed(dev, f0._build_pack)
        _lib.checked().nfx_made_affine_sample(packed, seed & ((1 << 64) - 1), state, z, cur, ld, num_samples, d,
                                              f0.conditioner.hidden_dim, _lib.stream_of(x))
        STATS["hip"] += 1
        with torch.no_grad():
            for i in range(1, n):
                nxt = x if (n - 1 - i) % 2 == 0 else spare
                self.flows[i]._hip_launch_counted(cur, nxt, ld, 1, accumulate=True)
                cur = nxt
        return x, ld, z

    def sample_on_device(self, num_samples, device="cuda", out=None):
        """z ~ N(0, I) drawn on the device and x, log_det = forward(z), for EVERY model whose
        no-grad fp32 forward runs the HIP chain: sample_fused where a kernel fuses the draw
        (sample_fused_ok); otherwise the stand-alone draw kernel (nfx_base_normal — the same
        values the fused kernels draw at that seed and offset) into z, then the forward chain on
        z. Between-layer BatchNorm in eval mode is a fixed map and is fine. Raises
        NotImplementedError only where forward itself would leave the HIP kernels (train-mode
        BatchNorm, a CPU device). Returns (x, log_det, z).
        out=(z, x, ld): caller buffers (contiguous, based at a 16-byte boundary, else ValueError);
        x and ld may be None (outside the fused path they are
        then the forward chain's own outputs, which saves two copies). Calls sharing this model's
        generator state must be stream-ordered."""
        dev = _cuda_device(device)
        if self.sample_fused_ok(num_samples, dev):
            if out is not None and (out[1] is None or out[2] is None):
                z = out[0]
                out = (z, torch.empty_like(z) if out[1] is None else out[1],
                       torch.empty(num_samples, device=dev) if out[2] is None else out[2])
            return self.sample_fused(num_samples, dev, out)
        if not self._sample_forward_ok(dev):
            raise NotImplementedError("sample_on_device: forward of this model does not run the HIP chain on "
                                      f"{dev} (train-mode BatchNorm, or not a ROCm device)")
        seed, state = self._sampler_state(dev)
        d = self.flows[0].data_dim
        z = torch.empty(num_samples, d, device=dev) if out is None else out[0]
        if (z.shape != (num_samples, d) or z.dtype != torch.float32 or z.device != dev or not z.is_contiguous()
                or z.data_ptr() & 15):
            raise ValueError(f"sample_on_device: z must be a contiguous fp32 [{num_samples}, {d}] tensor on {dev}, "
                             "based at a 16-byte boundary")
        _lib.checked().nfx_base_normal(seed & ((1 << 64) - 1), state, z, num_samples, d, _lib.stream_of(z))
        STATS["hip"] += 1
        with torch.no_grad():
            x, ld = self._hip_chain(z, 1)
            if out is not None and out[1] is not None:
                x = out[1].copy_(x)
            if out is not None and out[2] is not None:
                ld = out[2].copy_(ld)
        return x, ld, z

    def nll(self, x):
        """Mean negative log-likelihood, accumulated in float64 (python float)."""
        _, sums = self.log_prob(x, return_sums=True)
        s = sums.cpu()
        return -(s[0] / s[1]).item()


def _cuda_device(device):
    """torch.device(device) with the current index filled in for a bare "cuda"."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


_GAUSS_WS = collections.OrderedDict()
_GAUSS_WS_MAX = 8  # (device, stream) entries kept; least recently used dropped beyond


def gauss_workspace(B, device, stream=None):
    """The per-workgroup float64 partial sums + arrival word of the fused log_prob epilogues
    (nfx_gauss_workspace_bytes), cached per (device, stream). Any content is valid (ABI 3: the
    kernels tag the arrival word per launch). Launches on one stream are ordered; two streams
    never share a workspace (concurrent launches on one would race on its partials). The cache
    holds the _GAUSS_WS_MAX most recently used streams: a transient stream's entry is dropped
    once eight others were used after it (the caching allocator reuses a dropped buffer only on
    the stream it was allocated on, after that stream's queued work). Captured graphs
    (GraphedFlow, GraphedTrainStep) own theirs."""
    dev = torch.device(device)
    if dev.type == "cuda":
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        st = stream if stream is not None else torch.cuda.current_stream(idx)
        key = (dev.type, idx, int(st.cuda_stream))
    else:
        key = (dev.type, dev.index, 0)
    n = _lib.lib().nfx_gauss_workspace_bytes(B)
    ws = _GAUSS_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = new_gauss_workspace(B, dev)
        _GAUSS_WS[key] = ws
    _GAUSS_WS.move_to_end(key)
    while len(_GAUSS_WS) > _GAUSS_WS_MAX:
        _GAUSS_WS.popitem(last=False)
    return ws


def new_gauss_workspace(B, device):
    """A fresh log_prob workspace for B samples (for callers that own one). Any content is valid
    (ABI 3); nfx_gauss_workspace_init writes the clean arrival word up front (on the current
    stream), so even the first call skips the kernels' one-time claim of a foreign word."""
    ws = torch.empty(_lib.lib().nfx_gauss_workspace_bytes(B), device=device, dtype=torch.uint8)
    if ws.device.type == "cuda":
        _lib.checked().nfx_gauss_workspace_init(ws, _lib.stream_of(ws))
    return ws


def check_gauss_workspace(ws, B, device):
    n = _lib.lib().nfx_gauss_workspace_bytes(B)
    if ws.dtype != torch.uint8 or ws.device != torch.device(device) or ws.numel() < n or not ws.is_contiguous():
        raise ValueError(f"log_prob workspace: need a contiguous uint8 tensor of >= {n} bytes on {device}")
    if ws.data_ptr() & 15:  # float64 partials: a byte view at an odd offset of a larger buffer will not do
        raise ValueError("log_prob workspace: need a tensor based at a 16-byte boundary")
    return ws


def gauss_logprob(z, ld, logp=None, sums=None, ws=None):
    """Fused `MultivariateNormal(0,I).log_prob(z) + ld` and float64 [sum, count] (nfx_gauss_logprob)."""
    z, ld = _lib.dense(z), _lib.dense(ld)
    B, d = z.shape
    if logp is None:
        logp = torch.empty(B, device=z.device, dtype=torch.float32)
    if sums is None:
        sums = torch.empty(2, device=z.device, dtype=torch.float64)
    ws = gauss_workspace(B, z.device) if ws is None else check_gauss_workspace(ws, B, z.device)
    _lib.checked().nfx_gauss_logprob(z, ld, logp, sums, ws, B, d, _lib.stream_of(z))
    STATS["hip"] += 1
    return logp, sums


class _GaussLogProbFn(torch.autograd.Function):
    """log N(z; 0, I) + ld under autograd: nfx_gauss_logprob forward (the eval epilogue, the
    reference's rounding order), nfx_gauss_logprob_backward (dL/dz = -z g, dL/dld = g)."""

    @staticmethod
    def forward(ctx, z, ld, workspace):
        z = _lib.dense(z)
        logp, sums = gauss_logprob(z, _lib.dense(ld), ws=workspace)
        ctx.save_for_backward(z)
        ctx.mark_non_differentiable(sums)
        return logp, sums

    @staticmethod
    def backward(ctx, g, _gs):
        (z,) = ctx.saved_tensors
        B, d = z.shape
        g = _lib.dense(g.float())
        gz, gld = torch.empty_like(z), torch.empty_like(g)
        _lib.checked().nfx_gauss_logprob_backward(z, g, gz, gld, B, d, _lib.stream_of(z))
        STATS["hip"] += 1
        return gz, gld, None


# ---------------------------------------------------------------------------------------------
# Between-layer BatchNorm on the GPU (csrc/nfx_flowbn.hip)
# ---------------------------------------------------------------------------------------------
_FLOWBN_MAX_D = 1024


def _bn_hip_ok(x):
    return x.device.type == "cuda" and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] <= _FLOWBN_MAX_D


def _bn_launch(bn, x, out, ld, direction):
    """out = BN affine of x (running statistics), ld -+= the scalar log-det, in place."""
    B, d = x.shape
    _lib.checked().nfx_flowbn_apply(x, out, ld, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps),
                                    B, d, direction, _lib.stream_of(x))
    STATS["hip"] += 1


def _bn_workspace(B, d, device):
    return torch.empty(_lib.lib().nfx_flowbn_workspace_bytes(B, d), device=device, dtype=torch.uint8)


def _bn_update_running_hip(bn, x):
    """Train mode (normalizing_flow_model.py:74-79): fold the batch moments of x into the running
    statistics; with SyncBN enabled the moments are those of every rank's shard."""
    x = _lib.dense(x.detach())
    B, d = x.shape
    L = _lib.checked()
    stats = torch.empty(d, 3, device=x.device, dtype=torch.float64)
    ws = _bn_workspace(B, d, x.device)
    st = _lib.stream_of(x)
    L.nfx_flowbn_moments(x, B, d, stats, ws, st)
    merge_bn_stats(stats)
    momentum = bn.momentum if bn.momentum is not None else 0.1
    with torch.no_grad():
        L.nfx_flowbn_update_running(stats, bn.running_mean, bn.running_var, float(momentum), d, st)
        # the kernel writes the buffers behind autograd's back; bump their versions so every
        # version-keyed cache (packed images, graph strict checks) sees the change
        torch.autograd.graph.increment_version(bn.running_mean)
        torch.autograd.graph.increment_version(bn.running_var)
    STATS["hip"] += 2


def _synced_moments(x):
    """(mean, biased var) of x over every rank's shard (float64 Chan merge, cast to x's dtype)."""
    xd = x.detach().double()
    n = torch.full((x.shape[1],), float(x.shape[0]), dtype=torch.float64, device=x.device)
    mean = xd.mean(0)
    m2 = ((xd - mean) ** 2).sum(0)
    stats = torch.stack([n, mean, m2], dim=1)
    merge_bn_stats(stats)
    return stats[:, 1].to(x.dtype), (stats[:, 2] / stats[:, 0]).to(x.dtype)


def _as_ld(ld, x):
    """The running log-det sum as a [B] fp32 tensor (the reference starts it as the int 0)."""
    if isinstance(ld, torch.Tensor):
        return ld
    return torch.full((x.shape[0],), float(ld), device=x.device, dtype=x.dtype)


class _FlowBatchNormFn(torch.autograd.Function):
    """One between-layer BatchNorm call on the GPU with a HIP backward: (x, ld) -> (y, ld +- c)."""

    @staticmethod
    def forward(ctx, x, ld, weight, bias, bn, direction):
        x = _lib.dense(x)
        y = torch.empty_like(x)
        ld_out = ld.detach().to(torch.float32).contiguous().clone()
        _bn_launch(bn, x, y, ld_out, direction)
        ctx.direction = direction
        ctx.eps = float(bn.eps)
        ctx.save_for_backward(x, weight, bias, bn.running_mean.detach().clone(), bn.running_var.detach().clone())
        return y, ld_out

    @staticmethod
    def backward(ctx, gy, gld):
        x, weight, bias, rm, rv = ctx.saved_tensors
        B, d = x.shape
        gx = torch.empty_like(x)
        dg = torch.empty(d, device=x.device, dtype=torch.float32)
        db = torch.empty(d, device=x.device, dtype=torch.float32)
        gy = _lib.dense(gy) if gy is not None else None
        gld_c = _lib.dense(gld) if gld is not None else None
        ws = _bn_workspace(B, d, x.device)
        _lib.checked().nfx_flowbn_backward(x, gy, gld_c, gx, weight.detach(), bias.detach(), rm, rv, ctx.eps, dg, db,
                                           B, d, ctx.direction, ws, _lib.stream_of(x))
        STATS["hip"] += 1
        return gx, gld, dg, db, None, None
