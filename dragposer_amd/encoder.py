"""The pose-VAE encoder (reference autoencoder.py:56-143, skeleton.py:8-130,178-210), used once per
sequence to get the initial latent (drag_pose.py:47-51).  Plain PyTorch on the optimiser's device: three
[masked dense (kernel-size-1 SkeletonConv) -> SkeletonPool -> LeakyReLU(0.2)] stages 176->112->72->48, then
f_mu / f_logvar.  Not part of the per-frame hot path."""
import numpy as np
import torch

from .model import DEFAULT_MODEL


class PoseEncoder(torch.nn.Module):
    def __init__(self, model_path=DEFAULT_MODEL, arrays=None):
        super().__init__()
        raw = arrays if arrays is not None else np.load(model_path)
        t = lambda k: torch.tensor(np.asarray(raw[k]), dtype=torch.float32)
        for l in range(3):
            w = t(f"encoder.layers.{l}.0.weight")[..., 0] * t(f"encoder.layers.{l}.0.mask")[..., 0]  # skeleton.py:120
            self.register_buffer(f"conv_w{l}", w)
            self.register_buffer(f"conv_b{l}", t(f"encoder.layers.{l}.0.bias"))
            self.register_buffer(f"pool_w{l}", t(f"encoder.layers.{l}.1.weight"))
        self.register_buffer("mu_w", t("encoder.f_mu.weight"))
        self.register_buffer("mu_b", t("encoder.f_mu.bias"))
        self.register_buffer("lv_w", t("encoder.f_logvar.weight"))
        self.register_buffer("lv_b", t("encoder.f_logvar.bias"))

    def forward(self, pose):
        """pose [S, 176] normalised dual quaternions -> mu [S, 24], logvar [S, 24]"""
        h = pose
        for l in range(3):
            h = h @ getattr(self, f"conv_w{l}").T + getattr(self, f"conv_b{l}")
            h = h @ getattr(self, f"pool_w{l}").T
            h = torch.nn.functional.leaky_relu(h, 0.2)
        return h @ self.mu_w.T + self.mu_b, h @ self.lv_w.T + self.lv_b

    def sample(self, pose, generator=None, use_mean=False):
        """latent as the reference draws it: mu + eps * exp(0.5 logvar) (autoencoder.py:19-27)"""
        mu, logvar = self.forward(pose)
        if use_mean:
            return mu
        eps = torch.randn(mu.shape, generator=generator, device="cpu").to(mu.device)
        return mu + eps * torch.exp(0.5 * logvar)


class NativePoseEncoder:
    """The same encoder in one HIP launch (include/dragposer_encoder.h: dp_encode, dp_sequence_begin), for any number of poses.
    There is no CPU path: it needs an MI355X.  Tensors are contiguous fp32 on the encoder's device."""

    def __init__(self, model_path=DEFAULT_MODEL, arrays=None, device="cuda:0"):
        import ctypes as C

        from . import _lib

        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("NativePoseEncoder runs on an MI355X only (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _lib.load()
        model, _keep = _lib.encoder_model(arrays if arrays is not None else np.load(model_path))
        h = C.c_void_p()
        rc = self._lib.dp_encoder_create(C.byref(h), C.byref(model), self.device.index)
        if rc != _lib.DP_OK:
            raise _lib.DragPoserError(rc, (self._lib.dp_encoder_last_error(None) or b"").decode())
        self._h = h

    def geometry(self):
        """(poses per wavefront, wavefronts per workgroup, most workgroups of a launch)"""
        import ctypes as C

        g = [C.c_int() for _ in range(3)]
        self._check(self._lib.dp_encoder_geometry(self._h, *[C.byref(x) for x in g]))
        return tuple(x.value for x in g)

    def _check(self, rc):
        if rc != 0:
            from . import _lib

            raise _lib.DragPoserError(rc, (self._lib.dp_encoder_last_error(self._h) or b"").decode())

    def _in(self, t, width):
        t = torch.as_tensor(t, dtype=torch.float32, device=self.device).reshape(-1, width)
        return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.contiguous().clone()

    @staticmethod
    def _ptr(t):
        return t.data_ptr() if t is not None and t.numel() else None

    def encode(self, pose, eps=None, out=None, outputs=("mu", "logvar", "latent", "status")):
        """pose [n,176], eps [n,24] or None (latent = mu) -> dict of mu, logvar, latent [n,24] and status [n] (DP_STATUS_* bits).
        `out`: a dict of tensors to write into; `outputs`: which to compute when they are allocated here."""
        pose = self._in(pose, 176)
        n = pose.shape[0]
        eps = self._in(eps, 24) if eps is not None else None
        if eps is not None and eps.shape[0] != n:
            raise ValueError("eps must have one row per pose")
        if out is None:
            out = {k: torch.empty((n,) if k == "status" else (n, 24), dtype=torch.int32 if k == "status" else torch.float32, device=self.device)
                   for k in outputs}
        for k, t in out.items():
            want = (torch.int32, (n,)) if k == "status" else (torch.float32, (n, 24))
            if t.device != self.device or (t.dtype, tuple(t.shape)) != want or not t.is_contiguous():
                raise ValueError(f"out[{k!r}]: expected a contiguous {want[0]} tensor of shape {want[1]} on {self.device}")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = self._ptr
        self._check(self._lib.dp_encode(self._h, n, p(pose), p(eps), p(out.get("mu")), p(out.get("logvar")), p(out.get("latent")),
                                        p(out.get("status")), stream))
        return out

    def forward(self, pose):
        """pose [S,176] -> mu [S,24], logvar [S,24] (PoseEncoder.forward)"""
        o = self.encode(pose, outputs=("mu", "logvar"))
        return o["mu"], o["logvar"]

    __call__ = forward

    def sample(self, pose, generator=None, use_mean=False):
        """latent as the reference draws it (PoseEncoder.sample): eps from `generator` on the CPU"""
        n = torch.as_tensor(pose).reshape(-1, 176).shape[0]
        eps = None if use_mean else torch.randn((n, 24), generator=generator, device="cpu")
        return self.encode(pose, eps=eps, outputs=("latent",))["latent"]

    def begin(self, pose, eps, init_global_pos, init_global_rot, init_heights, history, status=None):
        """DragPose.set_initial_pose in one launch (dp_sequence_begin), into freshly allocated state tensors: returns a dict of latent [S,24],
        global_pos [S,3], global_rot [S,4], latent_buf [S,H,24], disp_buf [S,H,3], heights_buf [S,H,NH] and status [S]."""
        import ctypes as C

        from . import _lib

        pose = self._in(pose, 176)
        S = pose.shape[0]
        eps = self._in(eps, 24) if eps is not None else None
        gp, gr = self._in(init_global_pos, 3), self._in(init_global_rot, 4)
        hts = torch.as_tensor(init_heights, dtype=torch.float32, device=self.device).reshape(S, -1).contiguous()
        NH, H, dev = hts.shape[1], int(history), self.device
        if gp.shape[0] != S or gr.shape[0] != S or (eps is not None and eps.shape[0] != S):
            raise ValueError("eps and the initial position / rotation / heights must have one row per sequence")
        o = dict(latent=torch.empty(S, 24, device=dev), global_pos=torch.empty(S, 3, device=dev), global_rot=torch.empty(S, 4, device=dev),
                 latent_buf=torch.empty(S, H, 24, device=dev), disp_buf=torch.empty(S, H, 3, device=dev),
                 heights_buf=torch.empty(S, H, NH, device=dev), status=status if status is not None else torch.empty(S, dtype=torch.int32, device=dev))
        st = _lib.DpSeqState()
        st.global_pos, st.global_rot, st.latent_buf = o["global_pos"].data_ptr(), o["global_rot"].data_ptr(), o["latent_buf"].data_ptr()
        st.disp_buf, st.heights_buf, st.history, st.n_heights = o["disp_buf"].data_ptr(), o["heights_buf"].data_ptr(), H, NH
        stream = torch.cuda.current_stream(dev).cuda_stream
        p = self._ptr
        self._check(self._lib.dp_sequence_begin(self._h, S, p(pose), p(eps), p(gp), p(gr), p(hts), C.byref(st), p(o["latent"]), p(o["status"]), stream))
        return o

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.dp_encoder_destroy(h)
