"""``M5`` raw-waveform classifier with the reference's constructor, attribute names and state dict
(audio_models/M5/M5Net.py:4-38); eval-mode forward runs as one fused HIP kernel (ap_m5_fwd).  In train mode
(audio_models/M5/train.py:86-103) the forward uses batch statistics and the backward forms every parameter gradient and,
if asked, the waveform's (ap_m5_train_fwd / ap_m5_train_bwd); ``F.nll_loss`` and ``torch.optim`` stay torch's.
The class keeps the name ``M5`` because the eval scripts select ``transform=None`` by
``Classifier._get_name() == 'M5'`` (adaptive_attack_eval.py:90-93)."""
import ctypes as C

import torch
import torch.nn as nn

from ... import _native as N


class _M5InputGrad(torch.autograd.Function):
    """log-probabilities with the gradient w.r.t. the waveform formed by ap_m5_bwd (white_box_attack.py:392,437-439)."""

    @staticmethod
    def forward(ctx, x, mod):
        with torch.no_grad():
            out = mod.forward(x.detach())
        ctx.mod = mod
        ctx.save_for_backward(x.detach().float().contiguous())
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.detach().float().contiguous()
        dx = torch.empty_like(x)
        N.check(N.lib().ap_m5_bwd(ctx.mod._handle(), N.ptr(x), N.ptr(g), N.ptr(dx), x.shape[0], x.shape[2], N.stream()),
                "ap_m5_bwd")
        return dx, None


class _M5TrainFn(torch.autograd.Function):
    """Train-mode log-probabilities over (x, conv / bn / fc parameters): ap_m5_train_fwd leaves the four stages' pre-BatchNorm
    activations, pooled activations, selection bytes and batch statistics in a workspace, ap_m5_train_bwd turns them into the
    gradient blob (per stage conv.weight, conv.bias, bn.weight, bn.bias, then fc1.weight, fc1.bias) and dx."""

    @staticmethod
    def forward(ctx, x, mod, *params):
        out, saved = mod._train_forward(x, keep=True)
        ctx.mod, ctx.ws, ctx.shapes = mod, saved[2], [p.shape for p in params]
        ctx.save_for_backward(saved[0], saved[1])
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                              # create_graph=True reached this node
            raise NotImplementedError("audiopure_amd M5: no double backward through the train-mode step (create_graph=True)")
        x, blob = ctx.saved_tensors
        mod, lib = ctx.mod, N.lib()
        h = mod._train_handle()
        g = g.detach().float().contiguous()
        grads = torch.empty(lib.ap_m5_param_elems(h), device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        N.check(lib.ap_m5_train_bwd(h, N.ptr(blob), N.ptr(x), N.ptr(g), N.ptr(grads), N.ptr(dx), ctx.ws.data_ptr(),
                                    ctx.ws.numel(), x.shape[0], x.shape[2], N.stream()), "ap_m5_train_bwd")
        outs, o = [dx, None], 0
        for i, shape in enumerate(ctx.shapes):                   # each parameter its slice of the blob
            n = shape.numel()
            outs.append(grads[o:o + n].view(shape) if ctx.needs_input_grad[2 + i] else None)
            o += n
        return tuple(outs)


class M5(nn.Module):
    # Class-level defaults: the scripts obtain the classifier by un-pickling a whole module (audio_models/create_model.py:8-17),
    # which restores __dict__ without running __init__ -- a reference-pickled ``M5Net.M5`` lands here with the reference's
    # attributes only.
    _native = None
    _key = None
    _train_native = None                       # geometry-and-eps handle of the train-mode launchers (its folded images are never read)
    _train_key = None

    def __getstate__(self):                    # the device handle is rebuilt on demand, never pickled
        d = dict(self.__dict__)
        d.pop("_native", None)
        d.pop("_key", None)
        d.pop("_train_native", None)
        d.pop("_train_key", None)
        return d

    def __init__(self, n_input=1, first_kernel_size=80, n_output=35, stride=16, n_channel=32):
        super().__init__()
        if n_input != 1:
            raise NotImplementedError("audiopure_amd M5: n_input must be 1 (mono waveform)")
        self.conv1 = nn.Conv1d(n_input, n_channel, kernel_size=first_kernel_size, stride=stride)
        self.bn1 = nn.BatchNorm1d(n_channel)
        self.pool1 = nn.MaxPool1d(4)
        self.conv2 = nn.Conv1d(n_channel, n_channel, kernel_size=3)
        self.bn2 = nn.BatchNorm1d(n_channel)
        self.pool2 = nn.MaxPool1d(4)
        self.conv3 = nn.Conv1d(n_channel, 2 * n_channel, kernel_size=3)
        self.bn3 = nn.BatchNorm1d(2 * n_channel)
        self.pool3 = nn.MaxPool1d(4)
        self.conv4 = nn.Conv1d(2 * n_channel, 2 * n_channel, kernel_size=3)
        self.bn4 = nn.BatchNorm1d(2 * n_channel)
        self.pool4 = nn.MaxPool1d(4)
        self.fc1 = nn.Linear(2 * n_channel, n_output)

    def _tensors(self):
        ts = []
        for conv, bn in ((self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3), (self.conv4, self.bn4)):
            ts += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return ts + [self.fc1.weight, self.fc1.bias]

    def __del__(self):
        try:
            if self._native:
                N.lib().ap_m5_destroy(self._native)
        except Exception:
            pass
        try:
            if self._train_native:
                N.lib().ap_m5_destroy(self._train_native)
        except Exception:
            pass

    def _handle(self):
        ts = self._tensors()
        dev = ts[0].device
        if dev.type != "cuda":
            raise N.NativeError("audiopure_amd M5 needs its parameters on a HIP device (.cuda()); no CPU path")
        key = (dev, tuple((t._version, t.data_ptr()) for t in ts))
        if key != self._key:
            lib = N.lib()
            if self._native:
                lib.ap_m5_destroy(self._native)
                self._native = None
            blob = torch.cat([t.detach().reshape(-1).float() for t in ts]).contiguous()
            h = C.c_void_p()
            N.check(lib.ap_m5_create(self.fc1.out_features, self.conv1.out_channels, self.conv1.kernel_size[0],
                                     self.conv1.stride[0], float(self.bn1.eps), N.ptr(blob), blob.numel(), N.stream(),
                                     C.byref(h)), "ap_m5_create")
            self._native, self._key = h, key
        return self._native

    def _bns(self):
        return (self.bn1, self.bn2, self.bn3, self.bn4)

    def _params(self):
        ps = []
        for conv, bn in zip((self.conv1, self.conv2, self.conv3, self.conv4), self._bns()):
            ps += [conv.weight, conv.bias, bn.weight, bn.bias]
        return ps + [self.fc1.weight, self.fc1.bias]

    def _train_checks(self):
        """What the train-mode step does not serve, refused before anything is launched."""
        for bn in self._bns():
            if not bn.affine:
                raise NotImplementedError("audiopure_amd M5 train mode: BatchNorm1d(affine=False) is not served")
            if not bn.track_running_stats or bn.running_mean is None:
                raise NotImplementedError("audiopure_amd M5 train mode: BatchNorm1d(track_running_stats=False) is not served")
        if any(c.bias is None for c in (self.conv1, self.conv2, self.conv3, self.conv4)):
            raise NotImplementedError("audiopure_amd M5 train mode: convolutions without bias are not served")
        if any(t.device.type != "cuda" for t in self._tensors()):
            raise NotImplementedError("audiopure_amd M5 train mode needs its parameters on a HIP device (.cuda()); no CPU path")
        if len({float(bn.eps) for bn in self._bns()}) != 1:
            raise NotImplementedError("audiopure_amd M5 train mode: the four BatchNorm layers must share eps")

    def _train_handle(self, blob=None):
        dev = self.fc1.weight.device
        key = (dev, self.fc1.out_features, self.conv1.out_channels, self.conv1.kernel_size[0], self.conv1.stride[0], float(self.bn1.eps))
        if key != self._train_key:
            lib = N.lib()
            if self._train_native:
                lib.ap_m5_destroy(self._train_native)
                self._train_native = None
            if blob is None:
                blob = torch.cat([t.detach().reshape(-1).float() for t in self._tensors()]).contiguous()
            h = C.c_void_p()
            N.check(lib.ap_m5_create(key[1], key[2], key[3], key[4], key[5], N.ptr(blob), blob.numel(), N.stream(), C.byref(h)),
                    "ap_m5_create")
            self._train_native, self._train_key = h, key
        return self._train_native

    def _train_forward(self, x, keep):
        """Batch-statistics forward; updates the running statistics in place as nn.BatchNorm1d does (also under no_grad).
        -> (log-probabilities, (x, blob, workspace) for ap_m5_train_bwd or None)"""
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"expected [B,1,L], got {tuple(x.shape)}")
        bns = self._bns()
        moms = set()
        for bn in bns:                                           # momentum=None: the cumulative average, 1 / num_batches_tracked
            moms.add(1.0 / (int(bn.num_batches_tracked) + 1) if bn.momentum is None else float(bn.momentum))
        if len(moms) != 1:
            raise NotImplementedError("audiopure_amd M5 train mode: the four BatchNorm layers must share their momentum")
        lib = N.lib()
        x = x.detach().float().contiguous()
        blob = torch.cat([t.detach().reshape(-1).float() for t in self._tensors()]).contiguous()
        h = self._train_handle(blob)
        B, L = x.shape[0], x.shape[2]
        nbytes = lib.ap_m5_train_workspace_bytes(h, B, L)
        if nbytes == 0:
            N.check(-22, "ap_m5_train_workspace_bytes")
        ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
        out = torch.empty((B, self.fc1.out_features), device=x.device, dtype=torch.float32)
        nco = sum(bn.num_features for bn in bns)
        running = torch.empty(2 * nco, device=x.device, dtype=torch.float32)
        N.check(lib.ap_m5_train_fwd(h, N.ptr(blob), N.ptr(x), N.ptr(out), N.ptr(running), moms.pop(), ws.data_ptr(), nbytes,
                                    1 if keep else 0, B, L, N.stream()), "ap_m5_train_fwd")
        with torch.no_grad():                                    # in place: the buffers' _version moves, so the eval handle re-folds
            o = 0
            for bn in bns:
                n = bn.num_features
                bn.running_mean.copy_(running[o:o + n])
                bn.running_var.copy_(running[nco + o:nco + o + n])
                if bn.num_batches_tracked is not None:
                    bn.num_batches_tracked.add_(1)
                o += n
        return out, ((x, blob, ws) if keep else None)

    @N.on_device
    def forward(self, x):
        if self.training:
            self._train_checks()
            params = self._params()
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
                return _M5TrainFn.apply(x, self, *params)
            return self._train_forward(x, keep=False)[0]          # no_grad: batch statistics, running statistics move, nothing kept
        if torch.is_grad_enabled() and x.requires_grad:
            return _M5InputGrad.apply(x, self)                   # white-box attack: dL/dx (parameters frozen)
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"expected [B,1,L], got {tuple(x.shape)}")
        h = self._handle()
        x = x.detach().float().contiguous()
        out = torch.empty((x.shape[0], self.fc1.out_features), device=x.device, dtype=torch.float32)
        if x.shape[0] == 0:                                      # empty batch: empty scores, like the torch modules
            return out
        N.check(N.lib().ap_m5_fwd(h, N.ptr(x), N.ptr(out), x.shape[0], x.shape[2], N.stream()), "ap_m5_fwd")
        return out
