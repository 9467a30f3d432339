"""`DragPose`: the reference's stateful per-frame operator (python/src/drag_pose.py:12-414) for S
sequences advancing in lock-step, with the optimise loop dispatched to the HIP kernel.

What stays here (PyTorch-ROCm device tensors, a handful of tiny ops per frame):
  * the state the reference keeps between frames: latent, current global position /
    rotation, the 60-deep latent / displacement / height ring buffers, the temporal target buffer;
  * the temporal target block (row a12, drag_pose.py:234-294), which calls the Transformer;
  * nothing of the per-frame epilogue (row a11, drag_pose.py:369-402: global pose update, joint adjustment,
    buffer shifts, root channels of the returned pose): that is `dp_sequence_advance`, one launch on the state
    tensors held here.
What does not: decode / FK / loss / backward / Adam / the while-condition -- those run inside
`LatentOptimizer.optimize` (one kernel launch per frame index for all S sequences).

`run()` keeps the reference's argument names and meaning; tensors carry a leading sequence
dimension S (a single sequence may omit it, then the results omit it too, like the reference).
"""
import numpy as np
import torch

from .encoder import PoseEncoder
from .model import DEFAULT_MODEL, NJ
from .optimizer import LATENT, LatentOptimizer
from .temporal import HISTORY, PAST_FRAMES, SAMPLE_STEP


def arrays_from_generator_model(generator_model, offsets):
    """The reference's Generator_Model (generator_architecture.py: `.autoencoder`, `.data`, `.parents`) -> the array dict
    dragposer_amd.model.HostModel / PoseEncoder read (same keys as data/model_dancedb.npz).  `offsets` [22,3] is the
    skeleton's OFFSET table: the reference hands it to every run() (drag_pose.py:201); the context is created with it, and run(offsets=...)
    may still pass another performer's on any call."""
    sd = generator_model.autoencoder.state_dict()
    arrs = {k: v.detach().cpu().numpy() for k, v in sd.items()}
    d = generator_model.data
    arrs["means.dqs"], arrs["stds.dqs"] = d.mean_dqs.detach().cpu().numpy().reshape(-1), d.std_dqs.detach().cpu().numpy().reshape(-1)
    arrs["means.displacement"] = d.mean_displacement.detach().cpu().numpy().reshape(-1)
    arrs["stds.displacement"] = d.std_displacement.detach().cpu().numpy().reshape(-1)
    arrs["parents"] = np.asarray(generator_model.parents, dtype=np.int32)
    arrs["offsets"] = np.asarray(torch.as_tensor(offsets).detach().cpu(), dtype=np.float32).reshape(NJ, 3)
    return arrs


# what a frame step consumes of the kernel's results (the global rotation matrices `rot`, 198 floats per frame, are not among
# them: the kernel skips them when the pointer is NULL)
_RUN_OUTPUTS = ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters")


def _check_ar(temporal, ar, who):
    """what run(ar=) / run_frames(ar=) refuse before anything else"""
    if temporal is not None:
        raise ValueError(f"DragPose.{who}: ar= and a temporal model are two sources of the pull term's target; create the DragPose without one")
    if ar.order > HISTORY:
        raise ValueError(f"DragPose.{who}: ar.order {ar.order} exceeds the history of {HISTORY} frames")


def _solver_alone(who, **layers):
    """solver=LM(...) has the trackers, the pull and its own table (LM.terms) in its loss and nothing else (include/dragposer_lm.h, Not covered)"""
    for name, given in layers.items():
        if given is not None:
            raise ValueError(f"DragPose.{who}: solver= does not go with {name}= (include/dragposer_lm.h, Not covered)")


def _points_alone(terms, who, **layers):
    """a table with points (include/dragposer_points.h) runs through its own entry points, which take none of the sequence layers"""
    if terms is not None and getattr(terms, "has_points", False):
        for name, given in layers.items():
            if given is not None and given is not False:
                raise ValueError(f"DragPose.{who}: a table with points does not go with {name}= (include/dragposer_points.h, Not in)")


def _tracker_rows(trk, tp, tR):
    """E, the trackers of `trk`, after checking that the sparse targets [..., E, 3] / [..., E, 9] have one row each"""
    E = trk["mj"].numel()
    if tp.shape[-2] != E or tR.shape[-2] != E:
        raise ValueError("target_ee_pos / target_ee_rot / weights_joints must have one row per entry of mask_joints")
    return E


def _adjust(trk, joint_adjustment_indices, joint_adjustment_weight):
    """run()'s / run_frames()'s joint adjustment as the launches take it: (joint, target joint, weight) or None"""
    if joint_adjustment_indices is None:
        return None
    joint_index, ee_index = joint_adjustment_indices
    return (int(joint_index), int(trk["mj_host"][ee_index]), float(joint_adjustment_weight))


def _dense(trk, rows, fill=torch.zeros):
    """[T,S,E,...] rows in tracker-list order -> [T,S,22,...] per joint, the joints that are no trackers filled by `fill`"""
    dense = fill(rows.shape[:2] + (NJ,) + rows.shape[3:], dtype=rows.dtype, device=rows.device)
    return dense.index_copy_(2, trk["mj"], rows)


def _check_rows(terms, T, S):
    """a clip of T frames takes a term's `per_frame` as [S,4], held for all frames, or [T,S,4]"""
    for i, term in enumerate(terms.terms):
        if term.per_frame is not None and term.per_frame.dim() == 3 and int(term.per_frame.shape[0]) != T:
            raise ValueError(f"Terms: term {i}: per_frame must be [{S},4] or [{T},{S},4], got {tuple(term.per_frame.shape)}")


class DragPose:
    def __init__(self, generator_model, temporal_model, means_latent, stds_latent, device=None, device_gpu=None, n_sequences=1,
                 offsets=None, native_temporal=False, native_encoder=False):
        """Argument order of the reference (drag_pose.py:13).  `generator_model` is one of
          * a `LatentOptimizer` (an existing kernel context; `device` arguments are then ignored),
          * None / a path to a model .npz / a dict of its arrays (dragposer_amd.model) -- a context is created on
            `device_gpu` (or `device` if that names a GPU, else cuda:0),
          * the reference's own Generator_Model object, with `offsets` [22,3] (see arrays_from_generator_model).
        `n_sequences`: sequences advancing in lock-step (the reference: 1).  `native_temporal`: run the temporal target
        block (drag_pose.py:248-292) in one HIP launch (dp_temporal_predict) instead of PyTorch ops around nn.Transformer.
        `native_encoder`: set_initial_pose is one HIP launch (dp_sequence_begin, include/dragposer_encoder.h) instead of the PyTorch encoder."""
        if isinstance(generator_model, LatentOptimizer) or hasattr(generator_model, "host_model"):
            optimizer, arrays = generator_model, None
        else:
            dev = next((d for d in (device_gpu, device) if d is not None and torch.device(d).type == "cuda"), "cuda:0")
            if generator_model is None or isinstance(generator_model, str):
                arrays = None
                optimizer = LatentOptimizer(model_path=generator_model or DEFAULT_MODEL, device=dev)
            else:
                if isinstance(generator_model, dict):
                    arrays = generator_model
                else:
                    if offsets is None:
                        raise ValueError("a reference Generator_Model carries no bone offsets: pass offsets=[22,3]")
                    arrays = arrays_from_generator_model(generator_model, offsets)
                optimizer = LatentOptimizer(device=dev, arrays=arrays)
        self.opt = optimizer
        self._arrays = arrays
        self._encoder = None
        self._native_encoder = bool(native_encoder)
        self.device = optimizer.device
        self.temporal = temporal_model.to(self.device).eval() if temporal_model is not None else None
        self.S = int(n_sequences)
        dev = self.device
        hm = optimizer.host_model.arrays
        self.means_q = torch.from_numpy(hm["mean_q"]).to(dev)  # drag_pose.py:27-33
        self.stds_q = torch.from_numpy(hm["std_q"]).to(dev)
        self.offsets = torch.from_numpy(hm["offsets"]).to(dev)
        self.means_latent = torch.as_tensor(means_latent, dtype=torch.float32, device=dev)
        self.stds_latent = torch.as_tensor(stds_latent, dtype=torch.float32, device=dev)
        self.temporal_frames_index = list(PAST_FRAMES)
        self.target_latent_buffer = None
        self._native_temporal = None
        if native_temporal and self.temporal is not None:
            from .temporal import NativeTemporal

            self._native_temporal = NativeTemporal(self.temporal, self.means_latent, self.stds_latent, device=self.device)
        self.latent = None
        self.last = None
        self._idx_cache = {}
        self._trk_cache = {}
        self._out = [None, None]
        self._flip = 0
        self.hold_state = None  # [S,len(holds),4] (x, y, z, held) of run(holds=) / run_frames(holds=); zeroed when a sequence begins
        self.keep_latents = False  # True: run_frames also leaves every frame's latent in `last_latents` [T,S,24] (eval_drag --smooth reads it)
        self.lm_mu = None  # [S] the damping of run(solver=LM(...)) (include/dragposer_lm.h), kept from frame to frame; reset when a sequence begins
        self.gap_state = None  # [S,22,16] of run(gaps=) / run_frames(gaps=) (include/dragposer_gaps.h); zeroed when a sequence begins
        self.tether_state = None  # [S,len(tethers),8] of run(tethers=) / run_frames(tethers=) (include/dragposer_tethers.h); zeroed when a sequence begins
        self._skel_obj, self._skel_dev = None, None  # the last `offsets` object run() / run_frames() was given, and what it decided (_skeleton)

    def _holds(self, holds, terms, constraints, who):
        """run()'s / run_frames()'s `holds`: checked against the table, `hold_state` allocated (zeros: nothing held) on first use"""
        if holds is None:
            return
        if terms is None or constraints is not None:
            raise ValueError(f"DragPose.{who}: holds= refer to a table, pass terms= (Terms.from_constraints turns constraints into one)")
        holds.check(terms)
        if self.hold_state is None or tuple(self.hold_state.shape) != (self.S, len(holds), 4):
            self.hold_state = holds.new_state(self.S, self.device)

    def _tethers(self, tethers, terms, constraints, holds, who):
        """run()'s / run_frames()'s `tethers`: checked against the table and the holds, `tether_state` allocated (zeros: no path yet) on first use"""
        if tethers is None:
            return
        if terms is None or constraints is not None:
            raise ValueError(f"DragPose.{who}: tethers= refer to a table, pass terms= (Terms.from_constraints turns constraints into one)")
        tethers.check(terms, holds)
        if self.tether_state is None or tuple(self.tether_state.shape) != (self.S, len(tethers), 8):
            self.tether_state = tethers.new_state(self.S, self.device)

    def _index(self, values):
        """device index tensor for a Python list, created once (no host->device copy inside a captured step)"""
        key = tuple(int(v) for v in values)
        if key not in self._idx_cache:
            self._idx_cache[key] = torch.tensor(key, dtype=torch.int64, device=self.device)
        return self._idx_cache[key]

    def _skeleton(self, offsets):
        """run()'s / run_frames()'s `offsets` ([22,3] for every sequence, or [S,22,3]) -> None when they are the context's skeleton (rows
        1..21 within 1e-6: the plain launches, unchanged) or the fp32 device copy the skeleton launches read (include/dragposer_skeleton.h).
        Decided once per distinct object -- one host synchronisation then, none on the frames that pass the same object again; the object's
        contents are read at that point."""
        if offsets is None:
            return None
        if offsets is self._skel_obj:
            return self._skel_dev
        t = torch.as_tensor(offsets, dtype=torch.float32).to(self.device)
        if t.dim() == 2 and tuple(t.shape) == (NJ, 3):
            pass
        elif t.dim() == 3 and tuple(t.shape) == (self.S, NJ, 3):
            pass
        else:
            raise ValueError(f"offsets: expected [22,3] or [{self.S},22,3] bone offsets, got {tuple(t.shape)}")
        same = bool(torch.isclose(t[..., 1:, :], self.offsets[1:].expand_as(t[..., 1:, :]), atol=1e-6).all())  # (row 0 is ignored, as in dp_model)
        self._skel_obj, self._skel_dev = offsets, (None if same else t.contiguous().clone())
        return self._skel_dev

    # ------------------------------------------------------------------ state (drag_pose.py:47-64)
    def set_initial_pose(self, initial_pose, init_global_pos, initial_global_rot, initial_heights, eps=None, generator=None):
        """The reference's entry point (drag_pose.py:47): `initial_pose` (S,176,1) normalised dual quaternions ->
        latent = mu + eps * exp(logvar / 2) through the pose encoder (autoencoder.py:19-27,56-143), then the state of
        set_initial_state.  `eps` [S,24]: the normal draw to use (the reference takes it from torch's global generator);
        `generator`: a torch.Generator for the draw otherwise."""
        S = self.S
        if self._native_encoder:
            return self._begin_native(initial_pose, init_global_pos, initial_global_rot, initial_heights, eps, generator)
        if self._encoder is None:
            self._encoder = (PoseEncoder(arrays=self._arrays) if self._arrays is not None else PoseEncoder()).to(self.device)
        pose = torch.as_tensor(initial_pose, dtype=torch.float32, device=self.device).reshape(S, 176)
        with torch.no_grad():
            mu, logvar = self._encoder(pose)
            if eps is None:
                eps = torch.randn((S, LATENT), generator=generator)
            latent = mu + torch.as_tensor(eps, dtype=torch.float32).reshape(S, LATENT).to(self.device) * torch.exp(0.5 * logvar)
        self.set_initial_state(latent, init_global_pos, initial_global_rot, initial_heights)

    def _begin_native(self, initial_pose, init_global_pos, initial_global_rot, initial_heights, eps, generator):
        """set_initial_pose with native_encoder=True: eps drawn as above, then ONE launch that encodes and fills freshly allocated state"""
        from .encoder import NativePoseEncoder

        S = self.S
        if not isinstance(self._encoder, NativePoseEncoder):
            self._encoder = NativePoseEncoder(arrays=self._arrays, device=self.device) if self._arrays is not None else NativePoseEncoder(device=self.device)
        if eps is None:
            eps = torch.randn((S, LATENT), generator=generator)
        f = lambda t, width: torch.as_tensor(t, dtype=torch.float32, device=self.device).reshape(S, width)
        o = self._encoder.begin(f(initial_pose, 176), f(eps, LATENT), f(init_global_pos, 3), f(initial_global_rot, 4), f(initial_heights, -1), HISTORY)
        self.latent, self.current_global_pos, self.current_global_rot = o["latent"], o["global_pos"], o["global_rot"]
        self.latent_buffer, self.displacement_buffer, self.heights_buffer = o["latent_buf"], o["disp_buf"], o["heights_buf"]
        self.begin_status = o["status"]  # [S] DP_STATUS_* bits: non-zero where a sequence's initial pose / state was refused
        self.current_index = 0
        self.target_latent_buffer = None
        self.hold_state = None
        self.tether_state = None
        self.lm_mu = None
        self.gap_state = torch.zeros(self.S, NJ, 16, device=self.device)

    def set_initial_state(self, latent, init_global_pos, initial_global_rot, initial_heights):
        """What set_initial_pose leaves behind, with the initial latent given instead of encoded."""
        dev, S = self.device, self.S
        f = lambda t, shape: torch.as_tensor(t, dtype=torch.float32, device=dev).reshape(shape).clone()
        self.latent = f(latent, (S, LATENT))
        self.current_global_pos = f(init_global_pos, (S, 3))
        self.current_global_rot = f(initial_global_rot, (S, 4))
        self.latent_buffer = self.latent.unsqueeze(1).repeat(1, HISTORY, 1)
        self.displacement_buffer = torch.zeros(S, HISTORY, 3, device=dev)
        self.heights_buffer = f(initial_heights, (S, 1, -1)).repeat(1, HISTORY, 1)
        self.current_index = 0
        self.target_latent_buffer = None
        self.hold_state = None
        self.tether_state = None
        self.lm_mu = None
        self.gap_state = torch.zeros(self.S, NJ, 16, device=self.device)

    # ------------------------------------------------------------------ temporal target (drag_pose.py:234-294)
    def _temporal_targets(self, window):
        S, dev = self.S, self.device
        assert window % SAMPLE_STEP == 0
        if self.target_latent_buffer is None or self.target_latent_buffer.shape[1] != window + 1:
            if self.target_latent_buffer is not None:
                # a window CHANGED in the middle of a window restarts the window (a prediction is made this frame), as the native plug-in
                # does (dp_unity.cpp): the reference indexes the re-allocated buffer with the old index -- an IndexError when the window
                # shrank, rows of zeros until the next prediction when it grew -- and here the old index would make run_frames() ask
                # for a stretch of <= 0 frames
                self.current_index = 0
            self.target_latent_buffer = torch.zeros(S, window + 1, LATENT, device=dev)
        if self.current_index != 0 or self.temporal is None:  # no predictor: the buffer stays zero, use lambda_temporal = 0
            return
        if self._native_temporal is not None:
            self._native_temporal.predict(self.latent_buffer, self.displacement_buffer, self.heights_buffer, window,
                                          out=self.target_latent_buffer)
            return
        idx = self.temporal_frames_index
        idx_t = self._index(idx)
        with torch.no_grad():
            input_latent = self.latent_buffer.index_select(1, idx_t)[:, :-1].clone()
            input_disp = torch.stack([self.displacement_buffer[:, j:j + SAMPLE_STEP].sum(dim=1) for j in idx[:-1]], dim=1)
            tgt = self.latent_buffer[:, idx[-1]].unsqueeze(1).clone()
            input_latent = (input_latent - self.means_latent) / self.stds_latent
            tgt = (tgt - self.means_latent) / self.stds_latent
            heights = self.heights_buffer.index_select(1, idx_t)[:, :-1].clone()
            enc_in = torch.cat((input_latent, input_disp, heights), dim=-1)
            buf = self.target_latent_buffer
            for i in range(0, window + 1, SAMPLE_STEP):
                pred = self.temporal(enc_in, tgt)
                tgt = torch.cat((tgt, pred[:, -1:]), dim=1)
                buf[:, i] = pred[:, -1]
            buf = buf * self.stds_latent + self.means_latent
            for i in range(0, window, SAMPLE_STEP):  # "lerp" with weight 1: hold the next prediction
                buf[:, i:i + SAMPLE_STEP + 1] = buf[:, i + SAMPLE_STEP].unsqueeze(1)
            self.target_latent_buffer = buf

    # ------------------------------------------------------------------ one frame (drag_pose.py:196-414)
    def _trackers(self, mask_joints, weights_joints):
        """device copies of the tracker list and the dense per-joint weight / flag arrays of the C ABI, built once per
        distinct (mask_joints, weights_joints) -- they are the same objects frame after frame"""
        mj_h = np.asarray(mask_joints.cpu() if isinstance(mask_joints, torch.Tensor) else mask_joints, dtype=np.int64).reshape(-1)
        wj_h = np.asarray(weights_joints.cpu() if isinstance(weights_joints, torch.Tensor) else weights_joints, dtype=np.float32).reshape(-1, 2)
        key = (mj_h.tobytes(), wj_h.tobytes())
        if key not in self._trk_cache:
            if len(self._trk_cache) >= 8:  # a caller that keeps changing its tracker set: keep the cache bounded
                self._trk_cache.pop(next(iter(self._trk_cache)))
            dev, S = self.device, self.S
            if wj_h.shape[0] != mj_h.shape[0]:
                raise ValueError("target_ee_pos / target_ee_rot / weights_joints must have one row per entry of mask_joints")
            mj = torch.from_numpy(mj_h).to(dev)
            w = torch.zeros(S, NJ, 2, device=dev)
            tracked = torch.zeros(S, NJ, dtype=torch.uint8, device=dev)
            w.index_copy_(1, mj, torch.from_numpy(wj_h).to(dev).unsqueeze(0).expand(S, -1, -1).contiguous())
            tracked.index_fill_(1, mj, 1)
            # targets of untracked joints are never read, so the dense target arrays are allocated once and only the
            # tracked rows are rewritten every frame
            self._trk_cache[key] = dict(mj=mj, mj_host=mj_h, w=w, tracked=tracked, tgt_pos=torch.zeros(S, NJ, 3, device=dev),
                                        tgt_rot=torch.zeros(S, NJ, 9, device=dev))
        return self._trk_cache[key]

    @property
    def temporal_status(self):
        """DP_TEMPORAL_* bits of the native predictor's handle, read without synchronising (0 without one): 1 once a team of workgroups of an earlier
        prediction gave up waiting for a member -- that prediction's targets are NaN for the affected sequences (their frames then carry
        DP_STATUS_BAD_TARGETS in last_status), and the next prediction raises DragPoserError(DP_ERR_TIMEOUT) once before the operator goes on
        with one workgroup per sequence (include/dragposer.h: dp_temporal_status)"""
        return self._native_temporal.status() if self._native_temporal is not None else 0

    def _stretches(self, T, lambda_temporal, temporal_future_window):
        """A clip of T frames cut into the stretches between two temporal predictions: yields (t, n, z_tgt, strides, lambda_tmp) for one launch
        of frames t .. t + n each.  The reference predicts at current_index == 0 whatever lambda_temporal is (drag_pose.py:235-291), so the
        stretches are cut the same way with the pull term on or off; without a predictor there is nothing to pull towards, the clip is one
        stretch and the term is off, in run() and here alike (the reference cannot run without one).  The order is behaviour: the prediction
        is made right before its stretch is yielded, from the history buffers the launch before it advanced, and current_index moves when the
        caller comes back for the next stretch -- after its launch has returned, and not at all when that raised."""
        have = self.temporal is not None
        lambda_tmp = float(lambda_temporal) if have and float(lambda_temporal) != 0.0 else 0.0
        window = int(temporal_future_window)
        zero_tgt = torch.zeros(self.S, LATENT, device=self.device)
        t = 0
        while t < T:
            if have:  # frames up to the next prediction (a prediction every `window` frames; every frame when window = 0)
                self._temporal_targets(window)
                n = min(T - t, max(window, 1) - self.current_index)
                z_tgt, strides = self.target_latent_buffer[:, self.current_index:], (LATENT, (window + 1) * LATENT)
            else:
                n, z_tgt, strides = T - t, zero_tgt, (0, LATENT)
            yield t, n, z_tgt, strides, lambda_tmp
            t += n
            self.current_index = 0 if window == 0 else (self.current_index + n) % window

    def run_frames(self, target_ee_pos, target_ee_rot, mask_joints, weights_joints, target_root=None, stop_eps_pos=1e-2, stop_eps_rot=1e-2,
                   max_iter=100, min_loss_incr=0.00001, learning_rate=1e-3, lambda_rot=1, lambda_temporal=1, temporal_future_window=60,
                   height_indices=(0, 4, 8, 13, 17, 21), joint_adjustment_indices=None, joint_adjustment_weight=0.01, offsets=None,
                   constraints=None, terms=None, holds=None, ar=None, gaps=None, present=None, tethers=None, solver=None, _live=False):
        """T consecutive frames of every sequence -- T calls of run() -- with the frame loop on the device: one kernel launch per
        stretch of frames between two temporal predictions (all T of them when there is no predictor or lambda_temporal is 0).
        target_ee_pos [T,S,E,3], target_ee_rot [T,S,E,3,3]; `target_root` [T,S,3] or None: given, the position targets of frame t
        are target_ee_pos[t] + (target_root[t] - current_global_pos) as eval_drag builds them (eval_drag.py:186-199), which no
        caller can do ahead of time.  `offsets`: the performers' bone offsets as in run() -- [22,3] or [S,22,3], kept for all T frames.
        `constraints` (a dragposer_amd.Constraints) or `terms` (a dragposer_amd.Terms): the extra loss terms of run(constraints= / terms=)
        in every frame's loss, the frame loop still on the device (dp_optimize_sequence_constrained / dp_optimize_sequence_terms), cut
        into the same stretches and, unlike run(), together with `offsets`; a term's `per_frame` is [S,4], held for all T frames, or
        [T,S,4].  `last_terms` then holds the weighted terms of every frame ([T,S,4] / [T,S,len(terms)]) and `last_joint_pos` [T,S,22,3].
        `holds` (a dragposer_amd.Holds, with `terms`): joints held where they touched down (dp_optimize_sequence_holds,
        include/dragposer_holds.h); the state lives in `hold_state` [S,len(holds),4], zeroed when a sequence begins and passed through
        every stretch, and `last_hold_trace` [T,S,len(holds),4] holds it after every frame.
        `ar` (a dragposer_amd.LatentAR, for a DragPose without a temporal model): the pull term's target of every frame is the
        predictor's, formed from the sequence's own last latents inside ONE launch for all T frames (dp_optimize_sequence_ar,
        include/dragposer_latent_ar.h), weighed by `lambda_temporal`; with or without `terms`, `holds` and `offsets`, and `constraints`
        go through Terms.from_constraints (`last_terms` is then [T,S,len of that table]).  `last_z_tgt` [T,S,24] holds the targets used,
        `last_loss` [T,S,3] every frame's three loss parts.
        `gaps` (a dragposer_amd.Gaps): trackers that drop out and come back (dp_optimize_sequence_gaps, include/dragposer_gaps.h) -- a
        sample that is NaN, or whose entry of `present` [T,S,E] (tracker-list order; None: NaN samples alone mark gaps) is 0, is held at the
        joint's last good one for up to gaps.max_hold frames and leaves the loss after that.  With `ar` it is one launch, without it the
        usual stretches; the state lives in `gap_state` [S,22,16], zeroed when a sequence begins, and `last_gap_trace` [T,S,22] holds every
        joint's code of every frame (1 present, 2 held, 3 lost, 0 not a tracker).  Without `terms` it runs with an empty table, and
        `constraints` go through Terms.from_constraints, as with `ar`.
        A `terms` table with points (include/dragposer_points.h) runs through dp_optimize_sequence_terms_points, `offsets` allowed, none
        of `holds` / `ar` / `gaps` / `tethers`.
        `tethers` (a dragposer_amd.Tethers, with `terms`): joints tied to their own recent path (dp_optimize_sequence_tethers,
        include/dragposer_tethers.h), one launch per stretch, with or without `holds`, `ar` and `gaps` (without `gaps` it runs with
        Gaps(0, 1.0), under which an absent sample leaves the loss at once); the state lives in `tether_state` [S,len(tethers),8], zeroed
        when a sequence begins and passed through every stretch, and `last_tether_trace` [T,S,len(tethers),8] holds it after every frame.
        `solver` (a dragposer_amd.LM): every frame solved by Levenberg-Marquardt steps with the frame loop on the device
        (dp_optimize_sequence_lm, include/dragposer_sequence_lm.h), cut into the same stretches -- frame by frame the bits of run(solver=).
        `target_root` is honoured, `lm_mu` [S] is carried in place, `last_status`, `last_loss` [T,S,3] and `last_joint_pos` [T,S,22,3] are set.
        With `solver.predictor` (a dragposer_amd.LatentAR, for a DragPose without a temporal model) the pull term's target of every frame is
        formed inside ONE launch for all T frames, weighed by `lambda_temporal`, and `last_z_tgt` [T,S,24] holds the targets used.  With
        `solver.terms` (LM(3, terms=Terms([...])): a table without points; `per_frame` [S,4] or [T,S,4], offset per stretch as for Adam) the
        table's terms join the LM loss (dp_optimize_sequence_lm_terms, include/dragposer_sequence_lm_terms.h), `last_terms`
        [T,S,len(terms)] holds the weighted terms of every frame, and the frames are the bits of run(solver=) with that frame's table.  The
        table belongs to the solver as the predictor does: none of the other layers, `terms=` among them, goes with `solver=`.
        Returns (poses [T,S,88], global positions [T,S,3], iterations [T,S])."""
        if solver is not None:
            _solver_alone("run_frames", constraints=constraints, terms=terms, holds=holds, ar=ar, gaps=gaps, tethers=tethers, present=present)
            solver.check()
            if solver.predictor is not None:
                _check_ar(self.temporal, solver.predictor, "run_frames")
            if self._skeleton(offsets) is not None:
                raise ValueError("DragPose.run_frames: solver= runs on the context's skeleton only (include/dragposer_lm.h, Not covered)")
        if constraints is not None and terms is not None:
            raise ValueError("DragPose.run_frames: pass constraints or terms, not both")
        _points_alone(terms, "run_frames", holds=holds, gaps=gaps, ar=ar, tethers=tethers)
        if tethers is not None:
            self._tethers(tethers, terms, constraints, holds, "run_frames")
            if gaps is None:
                from .gaps import Gaps

                gaps = Gaps(0, 1.0)
        if ar is not None:
            _check_ar(self.temporal, ar, "run_frames")
        if gaps is None and present is not None:
            raise ValueError("DragPose.run_frames: present belongs to gaps=")
        if gaps is not None:
            gaps.check()
        if (ar is not None or gaps is not None) and constraints is not None:
            from .terms import Terms

            terms, constraints = Terms.from_constraints(constraints), None
        self._holds(holds, terms, constraints, "run_frames")
        dev, S = self.device, self.S
        skel = self._skeleton(offsets)
        tp = torch.as_tensor(target_ee_pos, dtype=torch.float32, device=dev)
        T = int(tp.shape[0])
        tp = tp.reshape(T, S, -1, 3)
        tR = torch.as_tensor(target_ee_rot, dtype=torch.float32, device=dev).reshape(T, S, -1, 9)
        trk = self._trackers(mask_joints, weights_joints)
        E = _tracker_rows(trk, tp, tR)
        dense_p, dense_r = _dense(trk, tp), _dense(trk, tR)
        root = torch.as_tensor(target_root, dtype=torch.float32, device=dev).reshape(T, S, 3).contiguous() if target_root is not None else None
        adjust = _adjust(trk, joint_adjustment_indices, joint_adjustment_weight)
        poses = torch.empty(T, S, 88, device=dev)
        gpos = torch.empty(T, S, 3, device=dev)
        iters = torch.empty(T, S, dtype=torch.int32, device=dev)
        status = torch.empty(T, S, dtype=torch.int32, device=dev)
        # (keep_latents: the launches' per-step scratch, whose first 24 columns are the step's latent, is kept instead of dropped)
        hist = torch.empty(T, S, LATENT + 3 + len(height_indices), device=dev) if self.keep_latents else None
        if solver is not None:
            self._run_frames_lm(solver, dense_p, dense_r, root, trk, adjust, poses, gpos, iters, status, stop_eps_pos, stop_eps_rot, lambda_rot,
                                lambda_temporal, temporal_future_window, height_indices, solver.terms, hist)
            if hist is not None:
                self.last_latents = hist[..., :LATENT].contiguous()
            return poses, gpos, iters
        with_terms = constraints is not None or terms is not None
        if with_terms:
            if terms is not None:
                _check_rows(terms, T, S)
            key, width = ("loss_extra", 4) if terms is None else ("loss_terms", len(terms))
            self.last_terms = torch.empty(T, S, width, device=dev)
            self.last_joint_pos = torch.empty(T, S, NJ, 3, device=dev)
        if holds is not None:
            self.last_hold_trace = torch.zeros(T, S, len(holds), 4, device=dev)
        if tethers is not None:
            self.last_tether_trace = torch.zeros(T, S, len(tethers), 8, device=dev)
        if ar is not None:
            self.last_z_tgt = torch.zeros(T, S, LATENT, device=dev)
        dense_here = None
        if gaps is not None:
            if self.gap_state is None:
                self.gap_state = gaps.new_state(S, dev)
            self.last_gap_trace = torch.zeros(T, S, NJ, dtype=torch.uint8, device=dev)
            if present is not None:
                here = torch.as_tensor(present, device=dev).reshape(T, S, -1)
                if here.shape[2] != E:
                    raise ValueError("present must have one entry per entry of mask_joints")
                dense_here = _dense(trk, (here != 0).to(torch.uint8), fill=torch.ones)

        def extra(t0, n):
            """the stretch's share of the layers' arguments: the table's rows, the per-step outputs and traces of frames t0 .. t0 + n"""
            kw = {}
            if with_terms:
                kw = {"constraints": constraints, "terms": terms.frames(t0, t0 + n) if terms is not None else None,
                      key: self.last_terms[t0:t0 + n], "joint_pos": self.last_joint_pos[t0:t0 + n]}
            if holds is not None:
                kw.update(holds=holds, hold_state=self.hold_state, hold_trace=self.last_hold_trace[t0:t0 + n])
            if tethers is not None:
                kw.update(tethers=tethers, tether_state=self.tether_state, tether_trace=self.last_tether_trace[t0:t0 + n])
            if gaps is not None:  # (`_live`: run(live=True)'s one frame, which the gap unit runs as ONE launch)
                kw.update(gaps=gaps, gap_state=self.gap_state, present=dense_here[t0:t0 + n] if dense_here is not None else None,
                          gap_trace=self.last_gap_trace[t0:t0 + n], live=_live)
            return kw

        # last_loss [T,S,3] of run_frames(gaps=) is filled stretch by stretch; run_frames(ar=)'s is the one its single launch allocates
        loss = torch.empty(T, S, 3, device=dev) if gaps is not None and ar is None else None

        def launch(t, n, z_tgt, strides, lambda_tmp, **kw):
            return self.opt.optimize_sequence(self.latent, dense_p[t:t + n], dense_r[t:t + n], root[t:t + n] if root is not None else None,
                                              trk["w"], trk["tracked"], z_tgt, strides, self.current_global_pos, self.current_global_rot,
                                              self.latent_buffer, self.displacement_buffer, self.heights_buffer, tuple(int(h) for h in height_indices),
                                              n_iter=max_iter, lr=learning_rate, lambda_rot=float(lambda_rot), lambda_tmp=lambda_tmp,
                                              stop_eps_pos=stop_eps_pos, stop_eps_rot=stop_eps_rot, min_loss_incr=min_loss_incr, adjust=adjust,
                                              pose_ret=poses[t:t + n], pos_ret=gpos[t:t + n], iters=iters[t:t + n], status=status[t:t + n], offsets=skel,
                                              loss=loss[t:t + n] if loss is not None else None, scratch=hist[t:t + n] if hist is not None else None,
                                              **extra(t, n), **kw)

        if ar is not None:  # one launch, no stretches: the targets come from inside it; the loss's third part is lambda_temporal times the pull towards last_z_tgt
            loss = launch(0, T, None, (0, 0), float(lambda_temporal), ar=ar, z_tgt_trace=self.last_z_tgt)["loss"]
        else:
            for stretch in self._stretches(T, lambda_temporal, temporal_future_window):
                launch(*stretch)
        self.last_status = status  # [T,S] DP_STATUS_* bits (include/dragposer.h): non-zero where a frame's inputs were not finite
        if loss is not None:
            self.last_loss = loss
        if hist is not None:
            self.last_latents = hist[..., :LATENT].contiguous()
        return poses, gpos, iters

    def _run_frames_lm(self, solver, dense_p, dense_r, root, trk, adjust, poses, gpos, iters, status, stop_eps_pos, stop_eps_rot, lambda_rot,
                       lambda_temporal, temporal_future_window, height_indices, terms=None, hist=None):
        """run_frames(solver=LM(...)) behind its preparation: the stretches of run_frames through dp_optimize_sequence_lm (with `terms`,
        dp_optimize_sequence_lm_terms); with a predictor, one launch"""
        dev, S, T = self.device, self.S, int(dense_p.shape[0])
        if terms is not None:
            _check_rows(terms, T, S)
            self.last_terms = torch.empty(T, S, len(terms), device=dev)
        loss = torch.empty(T, S, 3, device=dev)
        self.last_joint_pos = torch.empty(T, S, NJ, 3, device=dev)
        if self.lm_mu is None:
            self.lm_mu = torch.full((S,), float(solver.mu0), device=dev)
        heights = tuple(int(h) for h in height_indices)
        names = ("pose_ret", "pos_ret", "iters", "status", "loss", "joint_pos")

        def launch(t, n, z_tgt, strides, lam, **kw):
            if terms is not None:  # (the stretch's share of the table's rows and of its per-step output)
                kw.update(terms=terms.frames(t, t + n), loss_terms=self.last_terms[t:t + n])
            self.opt.optimize_sequence_lm(self.latent, dense_p[t:t + n], dense_r[t:t + n], root[t:t + n] if root is not None else None, trk["w"],
                                          trk["tracked"], z_tgt, strides, self.current_global_pos, self.current_global_rot, self.latent_buffer,
                                          self.displacement_buffer, self.heights_buffer, heights, lm=solver, lambda_rot=float(lambda_rot),
                                          lambda_tmp=lam, stop_eps_pos=stop_eps_pos, stop_eps_rot=stop_eps_rot, mu=self.lm_mu, adjust=adjust,
                                          pose_ret=poses[t:t + n], pos_ret=gpos[t:t + n], iters=iters[t:t + n], status=status[t:t + n],
                                          loss=loss[t:t + n], joint_pos=self.last_joint_pos[t:t + n], outputs=names,
                                          scratch=hist[t:t + n] if hist is not None else None, **kw)

        if solver.predictor is not None:  # one launch, no stretches: the targets come from inside it
            self.last_z_tgt = torch.zeros(T, S, LATENT, device=dev)
            launch(0, T, None, (0, 0), float(lambda_temporal), ar=solver.predictor, z_tgt_trace=self.last_z_tgt)
        else:  # (the stretches of run_frames, cut as for Adam)
            for stretch in self._stretches(T, lambda_temporal, temporal_future_window):
                launch(*stretch)
        self.last_status = status
        self.last_loss = loss
        return poses, gpos, iters

    def run(self, target_ee_pos, target_ee_rot, mask_joints, weights_joints, offsets=None, stop_eps_pos=1e-2,
            stop_eps_rot=1e-2, max_iter=100, min_loss_incr=0.00001, learning_rate=1e-3, lambda_rot=1, lambda_temporal=1,
            temporal_future_window=60, height_indices=(0, 4, 8, 13, 17, 21), joint_adjustment_indices=None,
            joint_adjustment_weight=0.01, verbose=False, out_pose=None, out_pos=None, constraints=None, terms=None, holds=None, ar=None,
            gaps=None, present=None, live=False, tethers=None, solver=None):
        """One frame for every sequence: one launch for the optimise loop and the epilogue, one for the history buffers, plus two
        row scatters of the targets.  `out_pose` [S,88] / `out_pos` [S,3]: optional caller storage for the returned tensors.
        `constraints` (a dragposer_amd.Constraints): the reference's extra loss terms (drag_pose.py:129-183) join the loss -- the frame
        is then dp_optimize_constrained followed by dp_sequence_advance (two launches), with this frame's current_global_pos as the
        floor term's global position; None runs the path above unchanged.  `terms` (a dragposer_amd.Terms): a table of user-defined
        terms instead, the same two launches with dp_optimize_terms (a term's per-frame rows: its [S,4] `per_frame` tensor, read at
        this call); not together with `constraints`.  `holds` (a dragposer_amd.Holds, with `terms`): each held term reads its row from
        `hold_state`, and the state is updated after the frame with include/dragposer_holds.h's arithmetic in torch on the device, no
        synchronisation -- frame by frame the bits of run_frames(terms=, holds=).  `ar` (a dragposer_amd.LatentAR): the frame is a one-step
        launch of run_frames(ar=), with everything that call takes (`offsets` together with `terms` included); frame by frame its bits.
        `gaps` (a dragposer_amd.Gaps) with `present` [S,E] or None: likewise a one-step run_frames(gaps=), with or without `ar`; `last`
        then holds the frame's `gap_trace` [S,22].
        `live` (with any of `constraints` / `terms` / `holds` / `ar` / `gaps`): that frame as ONE launch, dp_live_step
        (include/dragposer_live.h) -- the gap unit appends the frame's row to the history buffers itself; without `gaps` it runs with
        Gaps(0, 1.0), under which an absent sample leaves the loss at once.  The bits of the same call without `live`.
        A `terms` table with points (Terms(..., points=), include/dragposer_points.h) runs through dp_optimize_terms_points, with
        `offsets` allowed (dp_optimize_terms_points_skeleton) and none of `holds` / `ar` / `gaps` / `tethers` / `live`.
        `tethers` (a dragposer_amd.Tethers, with `terms`): the per-frame composition of include/dragposer_tethers.h -- each tethered term
        reads its row from `tether_state`, the frame is a one-step run_frames(gaps=) (Gaps(0, 1.0) without `gaps`), and the state is updated
        after it with the header's arithmetic in torch on the device, no synchronisation: frame by frame the bits of
        run_frames(terms=, tethers=).  Not together with `live`: dp_live_step has no tethers, run_frames(tethers=) is the one-launch form.
        `offsets`: the performer's bone offsets, as the reference takes them on every call (drag_pose.py:202) -- [22,3] for every sequence
        or [S,22,3] one per sequence.  The context's own skeleton (or None) runs the launches above unchanged; any other runs the same frame
        with those bones (dp_optimize_sequence_skeleton, include/dragposer_skeleton.h), not together with `constraints` / `terms`: this
        class does not route that combination; LatentOptimizer.optimize_constrained / optimize_terms take `offsets=` themselves.  Passing
        the same object frame after frame costs one host synchronisation in all (DragPose._skeleton).
        `solver` (a dragposer_amd.LM; None = Adam, the default): the frame's latent is found by Levenberg-Marquardt steps instead --
        dp_optimize_lm followed by dp_sequence_advance (two launches, include/dragposer_lm.h); max_iter, learning_rate and min_loss_incr are
        not used, stop_eps_pos / stop_eps_rot are the early stop's thresholds unless the LM carries its own.  The damping is kept per sequence
        in `lm_mu` [S] and reset when a sequence begins.  With `solver.predictor` (a dragposer_amd.LatentAR) the frame is a one-step launch of
        run_frames(solver=) instead (dp_optimize_sequence_lm), the pull's target formed from the sequence's last latents: its bits.  With `solver.terms`
        (LM(3, terms=Terms([...])), a table without points, `per_frame` [S,4]: this frame's rows) the table's terms join the LM loss:
        dp_optimize_lm_terms with this frame's current_global_pos, then dp_sequence_advance (two launches, include/dragposer_lm_terms.h), or
        with `solver.predictor` the one-step launch of run_frames(solver=); `last` then holds `loss_terms` [S,len(terms)].  Not together with
        constraints= / terms= / holds= / ar= / gaps= / tethers= / live= or offsets other than the context's skeleton: the table, like the
        predictor, belongs to the solver."""
        if solver is not None:
            _solver_alone("run", constraints=constraints, terms=terms, holds=holds, ar=ar, gaps=gaps, tethers=tethers, live=live or None,
                          present=present)
            solver.check()
            if self._skeleton(offsets) is not None:
                raise ValueError("DragPose.run: solver= runs on the context's skeleton only (include/dragposer_lm.h, Not covered)")
            if solver.predictor is not None:  # the one-step launch of run_frames(solver=): frame by frame its bits
                _check_ar(self.temporal, solver.predictor, "run")
                kw_frame = dict(stop_eps_pos=stop_eps_pos, stop_eps_rot=stop_eps_rot, lambda_rot=lambda_rot, lambda_temporal=lambda_temporal,
                                temporal_future_window=temporal_future_window, height_indices=height_indices,
                                joint_adjustment_indices=joint_adjustment_indices, joint_adjustment_weight=joint_adjustment_weight, solver=solver)
                return self._run_ar(target_ee_pos, target_ee_rot, mask_joints, weights_joints, out_pose, out_pos, verbose, kw_frame)
        if constraints is not None and terms is not None:
            raise ValueError("DragPose.run: pass constraints or terms, not both")
        _points_alone(terms, "run", holds=holds, gaps=gaps, ar=ar, tethers=tethers, live=bool(live))
        if tethers is not None:
            if live:
                raise ValueError("DragPose.run: live= has no tethers (dp_live_step); run_frames(tethers=) is their one-launch form")
            self._tethers(tethers, terms, constraints, holds, "run")
            if gaps is None:
                from .gaps import Gaps

                gaps = Gaps(0, 1.0)
        if live:
            if constraints is None and terms is None and holds is None and ar is None and gaps is None:
                raise ValueError("DragPose.run: live= goes with constraints=, terms=, holds=, ar= or gaps=")
            if gaps is None:
                from .gaps import Gaps

                gaps = Gaps(0, 1.0)
        if gaps is None and present is not None:
            raise ValueError("DragPose.run: present belongs to gaps=")
        if ar is not None or gaps is not None:
            if ar is not None:
                _check_ar(self.temporal, ar, "run")
            if gaps is not None:
                gaps.check()
                present = torch.as_tensor(present, device=self.device).reshape(1, self.S, -1) if present is not None else None
            kw_frame = dict(offsets=offsets, stop_eps_pos=stop_eps_pos, stop_eps_rot=stop_eps_rot, max_iter=max_iter,
                            min_loss_incr=min_loss_incr, learning_rate=learning_rate, lambda_rot=lambda_rot, lambda_temporal=lambda_temporal,
                            temporal_future_window=temporal_future_window, height_indices=height_indices,
                            joint_adjustment_indices=joint_adjustment_indices, joint_adjustment_weight=joint_adjustment_weight,
                            constraints=constraints, terms=terms, holds=holds, ar=ar, gaps=gaps, present=present,
                            _live=bool(live))  # (run_frames of this one frame: optimize_sequence(live=) launches dp_live_step)
            if tethers is not None:  # (tethered terms read this frame's state rows; the update follows the frame)
                kw_frame["terms"] = tethers.frame_terms(terms, self.tether_state)
            ret = self._run_ar(target_ee_pos, target_ee_rot, mask_joints, weights_joints, out_pose, out_pos, verbose, kw_frame)
            if tethers is not None:
                tethers.update(terms, self.tether_state, self.last_joint_pos[0], self.current_global_pos)
            return ret
        self._holds(holds, terms, constraints, "run")
        skel = self._skeleton(offsets)
        with_points = terms is not None and terms.has_points  # (routed with its bones: dp_optimize_terms_points_skeleton)
        if skel is not None and (constraints is not None or terms is not None) and not with_points:
            raise ValueError("DragPose.run: offsets other than the context's skeleton cannot be combined with " +
                             ("constraints=" if constraints is not None else "terms=") + " here: call LatentOptimizer.optimize_constrained / "
                             "optimize_terms with offsets= (dp_optimize_constrained_skeleton / dp_optimize_terms_skeleton), or create the "
                             "DragPose from this skeleton")
        dev, S = self.device, self.S
        squeeze = torch.as_tensor(target_ee_pos).dim() == 2
        tp = torch.as_tensor(target_ee_pos, dtype=torch.float32, device=dev).reshape(S, -1, 3)
        tR = torch.as_tensor(target_ee_rot, dtype=torch.float32, device=dev).reshape(S, -1, 9)
        trk = self._trackers(mask_joints, weights_joints)
        _tracker_rows(trk, tp, tR)

        self._temporal_targets(temporal_future_window)
        trk["tgt_pos"].index_copy_(1, trk["mj"], tp)
        trk["tgt_rot"].index_copy_(1, trk["mj"], tR)

        # one frame = a whole-sequence launch of one step (dp_optimize_sequence): the optimise loop AND run()'s epilogue
        # (drag_pose.py:369-402) in one kernel, the same one run_frames() uses for stretches of frames -- so cutting a sequence into
        # calls of run() or handing it to run_frames() whole gives the same bits
        adjust = _adjust(trk, joint_adjustment_indices, joint_adjustment_weight)
        pose = out_pose if out_pose is not None else torch.empty(S, 88, device=dev)
        gpos = out_pos if out_pos is not None else torch.empty(S, 3, device=dev)
        self._flip ^= 1  # two result sets, alternated: `last` stays valid while the next frame runs
        if self._out[self._flip] is None:
            self._out[self._flip] = dict(iters=torch.empty(1, S, dtype=torch.int32, device=dev), loss=torch.empty(1, S, 3, device=dev),
                                         status=torch.empty(1, S, dtype=torch.int32, device=dev),
                                         scratch=torch.empty(1, S, LATENT + 3 + len(height_indices), device=dev), z=torch.empty(S, LATENT, device=dev))
        o = self._out[self._flip]
        z_tgt = self.target_latent_buffer[:, self.current_index:]
        pull = self.temporal is not None and float(lambda_temporal) != 0.0  # (no predictor: the buffer is zeros, the term is off; run_frames() alike)
        if solver is not None:
            return self._run_lm(solver, trk, o, pose, gpos, adjust, height_indices, lambda_rot, lambda_temporal if pull else 0.0, stop_eps_pos,
                                stop_eps_rot, temporal_future_window, verbose, squeeze, solver.terms)
        if constraints is not None or terms is not None:
            return self._run_constrained(constraints if terms is None else terms, trk, o, pose, gpos, adjust, height_indices, max_iter, learning_rate, lambda_rot,
                                         lambda_temporal if pull else 0.0, stop_eps_pos, stop_eps_rot, min_loss_incr, temporal_future_window,
                                         verbose, squeeze, holds, skel if with_points else None)
        self.opt.optimize_sequence(self.latent, trk["tgt_pos"].unsqueeze(0), trk["tgt_rot"].unsqueeze(0), None, trk["w"], trk["tracked"], z_tgt,
                                   (0, (int(temporal_future_window) + 1) * LATENT), self.current_global_pos, self.current_global_rot,
                                   self.latent_buffer, self.displacement_buffer, self.heights_buffer, tuple(int(h) for h in height_indices),
                                   n_iter=max_iter, lr=learning_rate, lambda_rot=float(lambda_rot), lambda_tmp=float(lambda_temporal) if pull else 0.0,
                                   stop_eps_pos=stop_eps_pos, stop_eps_rot=stop_eps_rot, min_loss_incr=min_loss_incr, adjust=adjust,
                                   pose_ret=pose.unsqueeze(0), pos_ret=gpos.unsqueeze(0), iters=o["iters"], loss=o["loss"], scratch=o["scratch"],
                                   status=o["status"], offsets=skel)
        o["z"].copy_(self.latent)  # (self.latent is advanced in place by the next frame; `last` must not move with it)
        self.last = dict(iters=o["iters"][0], loss=o["loss"][0], z=o["z"], pose=pose, pos=gpos, status=o["status"][0])
        return self._end_frame(pose, gpos, verbose, squeeze, temporal_future_window)

    def _end_frame(self, pose, gpos, verbose, squeeze, window=None):
        """a frame's tail, `last` being set: the reference's printed line, current_index one frame on (`window` None: whoever ran the frame has
        moved it) and what run() returns -- without the sequence dimension for a single sequence that came without one"""
        if verbose:
            l, it = self.last["loss"].cpu(), self.last["iters"].cpu()
            print(f"Loss sqrt(Pos): {l[:, 0].sqrt().mean():.5f} // Loss Rot: {l[:, 1].mean():.5f} // "
                  f"Loss Temporal: {l[:, 2].mean():.5f} // Iter: {it.float().mean():.1f}")
        if window is not None:
            self.current_index = 0 if window == 0 else (self.current_index + 1) % window
        if squeeze and self.S == 1:
            return pose[0], gpos[0]
        return pose, gpos

    def _run_ar(self, target_ee_pos, target_ee_rot, mask_joints, weights_joints, out_pose, out_pos, verbose, kw):
        """run(ar=) / run(gaps=): run_frames(ar= / gaps=) on this one frame"""
        S = self.S
        squeeze = torch.as_tensor(target_ee_pos).dim() == 2
        tp = torch.as_tensor(target_ee_pos, dtype=torch.float32, device=self.device).reshape(1, S, -1, 3)
        tR = torch.as_tensor(target_ee_rot, dtype=torch.float32, device=self.device).reshape(1, S, -1, 3, 3)
        poses, gposs, iters = self.run_frames(tp, tR, mask_joints, weights_joints, **kw)
        pose, gpos = poses[0], gposs[0]
        if out_pose is not None:
            pose = out_pose.copy_(pose)
        if out_pos is not None:
            gpos = out_pos.copy_(gpos)
        self.last = dict(iters=iters[0], loss=self.last_loss[0], z=self.latent.clone(), pose=pose, pos=gpos, status=self.last_status[0])
        if kw.get("ar") is not None or kw.get("solver") is not None:
            self.last["z_tgt"] = self.last_z_tgt[0]
        if kw.get("gaps") is not None:
            self.last["gap_trace"] = self.last_gap_trace[0]
        return self._end_frame(pose, gpos, verbose, squeeze)  # (run_frames has moved current_index)

    def _run_lm(self, solver, trk, o, pose, gpos, adjust, height_indices, lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot, window, verbose, squeeze,
                terms=None):
        """run(solver=LM(...)): the frame's latent by dp_optimize_lm (with `terms`, dp_optimize_lm_terms reading the position before the frame),
        then run()'s epilogue (dp_sequence_advance)"""
        S = self.S
        if o.get("lm_frame") is None:
            o["lm_frame"] = self.opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
            o["lm_frame"].update(n_accepted=torch.empty(S, dtype=torch.int32, device=self.device), loss0=torch.empty(S, 3, device=self.device))
        fr = o["lm_frame"]
        if self.lm_mu is None:
            self.lm_mu = torch.full((S,), float(solver.mu0), device=self.device)
        z_tgt = self.target_latent_buffer[:, self.current_index].contiguous()
        names = tuple(fr) + ("mu",) + (("loss_terms",) if terms is not None else ())
        got = self.opt.optimize_lm(self.latent, z_tgt, self.current_global_rot, trk["tgt_pos"], trk["tgt_rot"], trk["w"], trk["tracked"], lm=solver,
                                   lambda_rot=float(lambda_rot), lambda_tmp=float(lambda_tmp), mu=self.lm_mu, stop_eps_pos=stop_eps_pos,
                                   stop_eps_rot=stop_eps_rot, out=fr, outputs=names, terms=terms,
                                   global_pos=self.current_global_pos if terms is not None else None)
        self.opt.sequence_advance(fr, self.current_global_pos, self.current_global_rot, self.latent_buffer, self.displacement_buffer,
                                  self.heights_buffer, tuple(int(h) for h in height_indices), pose_ret=pose, pos_ret=gpos, adjust=adjust,
                                  tgt_pos=trk["tgt_pos"] if adjust is not None else None)
        self.latent.copy_(fr["z"])
        o["z"].copy_(self.latent)
        self.last = dict(iters=fr["iters"], loss=fr["loss"], z=o["z"], pose=pose, pos=gpos, status=fr["status"], n_accepted=fr["n_accepted"],
                         loss0=fr["loss0"], joint_pos=fr["pos"])
        if terms is not None:
            self.last["loss_terms"] = got["loss_terms"]
        return self._end_frame(pose, gpos, verbose, squeeze, window)

    def _run_constrained(self, constraints, trk, o, pose, gpos, adjust, height_indices, max_iter, learning_rate, lambda_rot, lambda_tmp,
                         stop_eps_pos, stop_eps_rot, min_loss_incr, window, verbose, squeeze, holds=None, skel=None):
        """run()'s frame with extra loss terms: the optimise loop (dp_optimize_constrained for a Constraints, dp_optimize_terms for a
        Terms table) and run()'s epilogue (dp_sequence_advance)"""
        from .terms import Terms

        S = self.S
        table = isinstance(constraints, Terms)
        if o.get("frame") is None:
            o["frame"] = self.opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
        fr = o["frame"]
        key, width = ("loss_terms", len(constraints)) if table else ("loss_extra", 4)
        fr.pop("loss_terms" if not table else "loss_extra", None)
        if fr.get(key) is None or fr[key].shape[1] != width:
            fr[key] = torch.empty(S, width, device=self.device)
        z_tgt = self.target_latent_buffer[:, self.current_index].contiguous()
        run = self.opt.optimize_terms if table else self.opt.optimize_constrained
        table_in = constraints
        if holds is not None:  # (held terms read this frame's state rows; the update follows the epilogue)
            constraints = holds.frame_terms(table_in, self.hold_state)
        run(self.latent, z_tgt, self.current_global_rot, trk["tgt_pos"], trk["tgt_rot"], trk["w"], trk["tracked"], constraints,
            global_pos=self.current_global_pos, n_iter=max_iter, lr=learning_rate, lambda_rot=float(lambda_rot), lambda_tmp=float(lambda_tmp),
            stop_eps_pos=stop_eps_pos, stop_eps_rot=stop_eps_rot, min_loss_incr=min_loss_incr, out=fr, outputs=tuple(fr),
            **({} if skel is None else {"offsets": skel}))
        self.opt.sequence_advance(fr, self.current_global_pos, self.current_global_rot, self.latent_buffer, self.displacement_buffer,
                                  self.heights_buffer, tuple(int(h) for h in height_indices), pose_ret=pose, pos_ret=gpos, adjust=adjust,
                                  tgt_pos=trk["tgt_pos"] if adjust is not None else None)
        self.latent.copy_(fr["z"])
        if holds is not None:
            holds.update(table_in, self.hold_state, fr["pos"], self.current_global_pos)
        o["z"].copy_(self.latent)
        self.last = dict(iters=fr["iters"], loss=fr["loss"], z=o["z"], pose=pose, pos=gpos, status=fr["status"])
        self.last[key] = fr[key]
        if table:
            self.last["joint_pos"] = fr["pos"]  # [S,22,3] P_j of the frame (world: the current_global_pos before the call + P_j)
        return self._end_frame(pose, gpos, verbose, squeeze, window)
