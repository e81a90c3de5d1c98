"""Thin multimodal training step: render, losses, backward, optimiser.  The loss terms themselves live in
nvsf/nerf/losses.py (the Python half of csrc/losses.hip), whole-frame evaluation and its metrics in nvsf/nerf/evaluate.py.

Only what sits directly around the hot path, restated from the reference's `Trainer.train_step`
(nvsf/nerf/trainer.py:153-656) with the default CLI settings of nvsf/scripts/main_nvsf.py:60-97:
  * the sum of the loss parts (trainer.py:540-543): the LiDAR and camera terms of losses.py, the chamfer distance between the predicted
    and the true point cloud, `(d1 + d2).mean() * 0.5` (trainer.py:229-233; it IS part of the total at :542), on csrc/chamfer.hip, the
    optional scene-flow loss (`--flow_loss`, trainer.py:236-267); NaN -> 0, Inf -> 1e5 on the scalar (trainer.py:545-546);
  * optimiser: Adam(betas 0.9/0.99, eps 1e-15) on `model.get_params(lr)` and the 0.1^(iter/iters) decay
    (main_nvsf.py:350-362), under the GradScaler of the reference's fp16 run (trainer.py:119, 1332-1334);
  * EMA of the weights, decay 0.95, updated once per epoch (trainer.py:112-114, 1420-1421; nvsf/nerf/ema.py).
Across GPUs the step is frame-sharded: every rank renders its own frame, then ONE bucketed gradient all-reduce
(nvsf/frame_shard.py).  Checkpoints use the reference's dict (utils.py:622-747).
Shipped-config extras (configs/kitti360_1908.txt:13-15 `grad_loss`, `use_error_map`): the alternation between random pixels and LiDAR
patches (trainer.py:1035-1062: `set_epoch`) and the write-back into the error maps the patch sampler draws from (`update_error_maps`).
The regulariser's three smoothness switches fail in the reference itself (see __init__).  Logging is out of scope; the U-Net ray-drop
refinement lives in nvsf/nerf/refine.py.
"""
import warnings

import torch

from nvsf import frame_shard
from nvsf.nerf.losses import (DEFAULT_CRITERIA, CameraCritLossFn, CameraLossFn, CritSumFn, DistortionLossFn, LidarCritLossFn, LidarGradLossFn,
                              LidarLossFn, MseSumFn, UrfLossFn, lidar_losses_host, per_ray_criterion, rgb_depth_loss_host, rgb_loss_host,
                              update_error_map, urf_line_of_sight_loss)
from nvsf.nerf.losses import distortion_loss as distortion_loss_host


class RenderTrainStep:
    def __init__(self, model, lr=1e-2, iters=30000, num_steps=768, alpha_d=1.0, alpha_r=0.01, alpha_i=0.1, alpha_rgb=1.0,
                 smooth_factor=0.0, use_urf_loss=False, bucket_bytes=64 << 20, fp16=True, scale=1.0, chamfer_loss=True,
                 flow_loss=False, pc_list=None, ema_decay=0.95, split_backward=True, ray_chunks=1, grad_loss=False, depth_grad_loss="l1",
                 alpha_grad=0.1, patch_size_lidar=1, change_patch_size_lidar=(2, 8), change_patch_size_epoch=2, use_error_map=False,
                 sobel_grad=False, grad_norm_smooth=False, spatial_smooth=False, tv_loss=False, use_rgbd_loss=False, rgb_depth_loss="l1",
                 alpha_rd=1.0, depth_loss="l1", raydrop_loss="mse", intensity_loss="mse", rgb_loss="mse", upsample_steps=0, distortion_loss=False,
                 alpha_dist=0.01):
        """Defaults = the reference's CLI defaults (main_nvsf.py:60-97).  `scale`: the scene scale the chamfer loss divides by
        (opt.scale); `pc_list`: {frame index: [P, 3] tensor} world-frame point clouds for the scene-flow loss
        (Trainer.process_pointcloud, trainer.py:1848-1912, builds them from the range images); `ema_decay=None` disables EMA.
        `split_backward`: the LiDAR terms and the camera term of the loss are sums over disjoint ray sets, so their gradients add:
        the step runs camera forward + backward, then LiDAR forward + backward, and the camera table scatter (the longest kernel
        of the step, on its side stream) overlaps the whole LiDAR pass instead of the tail of one joint backward.  Same
        gradients (test_train_step_gpu.py); the reference's `nan_to_num` of the total is applied per modality, which differs
        only when a loss is not finite (then that modality contributes no gradient; GradScaler skips such a step anyway).
        `use_rgbd_loss`, `rgb_depth_loss`, `alpha_rd` (main_nvsf.py:84, 91, 97): the camera depth term against the LiDAR-projected
        depth map batch["gt_rgb_depth"] (FrameSet(camera_depth=True)); switched on, both camera terms are one launch (CameraLossFn).
        `depth_loss`, `raydrop_loss`, `intensity_loss`, `rgb_loss` (main_nvsf.py:83-88): the criterion of each per-ray term, one of
        l1 / mse / huber / smoothl1 / bce; the defaults go through the entries they always did, anything else through the `_crit`
        entries of csrc/losses.hip (and the error maps follow).
        `upsample_steps` (main_nvsf.py:73) above 0: both modalities are rendered with `hierarchical=True, upsample_steps=...`
        (NeRFRenderer.run: that many more samples per ray, drawn from the coarse weights); the line-of-sight loss then reads the
        merged rows.  0, the default, leaves the step as it is.
        `distortion_loss`, `alpha_dist`: the distortion loss of mip-NeRF 360 (the regulariser the reference sketched and left commented
        out at renderer_dynamic.py:242-245: O(T^2) as written there) on the rows both renders return, [N, T] or [N, T + U]:
        parts "dist_lidar" and "dist", alpha_dist x the mean over the rays (losses.DistortionLossFn on the device, losses.distortion_loss
        on the host).  Off, the default, leaves the step as it is."""
        self.model = model
        self.distortion, self.alpha_dist = bool(distortion_loss), float(alpha_dist)
        if self.distortion and getattr(model, "cuda_ray", False):
            raise ValueError("distortion_loss=True reads the [N, T] rows of weights and z_vals, which the occupancy-grid path (run_cuda) "
                             "does not return: train this model with distortion_loss=False, or without its occupancy grid")
        self.upsample_steps = int(upsample_steps)
        if self.upsample_steps < 0:
            raise ValueError(f"upsample_steps is a sample count, got {upsample_steps}")
        if self.upsample_steps > 0:
            from nvsf import field_ops as _ops
            _ops.check_resample_sizes(num_steps, self.upsample_steps)  # fails here, not at the first step
            if getattr(model, "cuda_ray", False):
                raise ValueError("upsample_steps > 0 renders with hierarchical=True, which the occupancy-grid path (run_cuda) "
                                 "does not do: train this model with upsample_steps=0, or without its occupancy grid")
        self._resample_kw = {"hierarchical": True, "upsample_steps": self.upsample_steps} if self.upsample_steps > 0 else {}
        self.criteria = {"depth_loss": str(depth_loss), "raydrop_loss": str(raydrop_loss), "intensity_loss": str(intensity_loss),
                         "rgb_loss": str(rgb_loss)}
        for option, name in self.criteria.items():
            per_ray_criterion(option, name, scale)  # an unknown criterion (or "cos") fails here, with the option named
        lidar = tuple(self.criteria[k] for k in ("depth_loss", "raydrop_loss", "intensity_loss"))
        # None = the default criteria: the entries and host expressions without a criterion argument
        self.lidar_criteria = None if all(self.criteria[k] == DEFAULT_CRITERIA[k] for k in ("depth_loss", "raydrop_loss", "intensity_loss")) else lidar
        self.rgb_criterion = None if self.criteria["rgb_loss"] == DEFAULT_CRITERIA["rgb_loss"] else self.criteria["rgb_loss"]
        self.use_rgbd_loss, self.rgb_depth_loss, self.alpha_rd = bool(use_rgbd_loss), str(rgb_depth_loss), float(alpha_rd)
        if self.use_rgbd_loss:
            CameraLossFn.criterion_code(self.rgb_depth_loss, scale)  # an unknown criterion (or "cos") fails here, not at the first step
        # loss scaling of the reference's mixed-precision run (trainer.py:119, 1332-1334: GradScaler(enabled=fp16) -> scale(loss)
        # .backward() -> step -> update; `-L` / `--fp16` in main_nvsf.py:17,43,159).  The encoders hand fp16 features to the
        # MLPs, so the gradients that travel back between them are fp16 tensors.
        # LossScaler = GradScaler's rule, state_dict and kernels; it lets the step decide about an overflow before the last table
        # scatter has finished (nvsf/nerf/loss_scaler.py)
        from nvsf.nerf.loss_scaler import LossScaler
        self.scaler = LossScaler(enabled=bool(fp16) and torch.cuda.is_available())
        if fp16 and hasattr(model, "flow_net"):
            model.flow_net.flow_mlp_mode = "fused"  # the flow MLP as autocast runs it: fp16 MFMA kernels (flow_field.FlowMlpFn)
        # Adam as one HIP pass per parameter tensor with the scaler's overflow flag consumed on the device (nvsf/nerf/adam.py).
        # torch's own fused=True variant was tried first: under this eps = 1e-15 / GradScaler setting it trains measurably worse
        # (tests/test_train_step_gpu.py: loss 0.289 -> 0.258 after 120 steps against 0.227).
        on_gpu = torch.cuda.is_available() and next(model.parameters()).is_cuda
        if on_gpu:
            from nvsf.nerf.adam import FusedAdam
            self.opt = FusedAdam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15)
        else:  # host-side logic tests only (checkpoint schema, gloo): the product path above needs the HIP device
            self.opt = torch.optim.Adam(model.get_params(lr), betas=(0.9, 0.99), eps=1e-15)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda it: 0.1 ** min(it / iters, 1))
        self.iters, self.num_steps = iters, num_steps
        self.alpha_d, self.alpha_r, self.alpha_i, self.alpha_rgb = alpha_d, alpha_r, alpha_i, alpha_rgb
        self.smooth, self.use_urf, self.bucket_bytes = smooth_factor, use_urf_loss, bucket_bytes
        self.scale, self.use_chamfer, self.use_flow, self.pc_list = float(scale), bool(chamfer_loss), bool(flow_loss), pc_list or {}
        # structural regularisation on LiDAR patches + the error maps of the patch sampler (main_nvsf.py:79-111 defaults; the shipped
        # config switches grad_loss and use_error_map on, configs/kitti360_1908.txt:13-14)
        self.grad_loss, self.depth_grad_loss, self.alpha_grad = bool(grad_loss), str(depth_grad_loss), float(alpha_grad)
        self.sobel_grad = bool(sobel_grad)
        if grad_norm_smooth or spatial_smooth or tv_loss:
            # trainer.py:337-350 add a [num_patch, 1, pH, pW] tensor to the loss, so that `loss` is no scalar any more and
            # scaler.scale(loss).backward() (trainer.py:1332) raises: the three switches cannot be trained with in the reference
            raise NotImplementedError("grad_norm_smooth / spatial_smooth / tv_loss make the reference's loss a non-scalar tensor "
                                      "(trainer.py:337-350, 543-545) that its own backward call rejects; there is no behaviour to match")
        self.patch_size_lidar = patch_size_lidar
        self.change_patch_size_lidar, self.change_patch_size_epoch = tuple(change_patch_size_lidar), int(change_patch_size_epoch)
        self.use_error_map, self.pixel_sampler = bool(use_error_map), "random"
        self.error_maps = None   # the FrameSet whose error_map / error_map_rgb the step keeps up to date (attach_error_maps)
        self._for_error_map = {}
        self.ema = None
        if ema_decay is not None and on_gpu:
            from nvsf.nerf.ema import ExponentialMovingAverage
            self.ema = ExponentialMovingAverage(model.parameters(), decay=ema_decay)
            self.ema.before_access = self.sync  # evaluate_frames(ema=step.ema) right after step(): store / copy_to / restore wait
        self._cham = None
        self.global_step = 0
        self.failed_to_load = []  # components of the last load_checkpoint whose state could not be restored
        self.scatter_overlap = True  # table scatters on a side stream beside the rest of backward (field_ops.scatter_to_sink)
        self.split_backward = bool(split_backward)
        self.ray_chunks = max(1, int(ray_chunks))
        # more than one rank: gradients live in flat buckets that are all-reduced while backward still runs (frame_shard.GradBuckets)
        # what the table-scatter nodes of the model need to know about this step (gradient sink, side-stream overlap, scatters still
        # expected: field_ops.announce / scatter_to_sink): an object of the step, attached to the model -- not process-wide state
        from nvsf import field_ops
        self.train_ctx = field_ops.TrainContext()
        for mod in model.modules():
            mod.__dict__["_train_ctx"] = self.train_ctx
        self.buckets = None
        if frame_shard.world()[1] > 1:
            self.buckets = frame_shard.GradBuckets([p for g in self.opt.param_groups for p in g["params"]], bucket_bytes, train_ctx=self.train_ctx)
        # One process: the optimiser pass of the table whose scatter ran LAST is issued on that scatter's stream, behind it, and the
        # main stream goes on with the next step (whose first pass -- the camera's -- does not read that table): `defer_last_table`.
        self.defer_last_table = on_gpu and self.buckets is None
        self._sink = None
        self._pending = None  # (event behind the deferred optimiser pass, its parameters)
        self._late_carry = None  # overflow found ONLY in a deferred table's gradient: reaches the scaler one step later (step())
        if self.defer_last_table:
            # a direct model.state_dict() / optimiser state_dict right after step() must see the deferred pass finished as well
            # (the fp16-cache and K-planes readers wait by themselves; fp32 readers outside this package go through these hooks)
            import weakref
            me = weakref.ref(self)
            settle = lambda *a, **k: (me() is not None and me().sync()) and None
            model.register_state_dict_pre_hook(settle)
            self.opt.register_state_dict_pre_hook(lambda *a, **k: settle())
        # parameter -> the Planes4D module that owns it (its kernels read the fp32 parameter: planes_field.Planes4D.wait_pending_update)
        self._plane_owner = {mod.planes_cl: mod for mod in model.modules() if isinstance(getattr(mod, "planes_cl", None), torch.nn.Parameter)}
        self._cache_of = {}   # parameter -> the fp16 cache of the module that owns it (tinycudann.Encoding / Network)
        for mod in model.modules():
            if hasattr(mod, "_cache") and isinstance(getattr(mod, "params", None), torch.nn.Parameter):
                self._cache_of[mod.params] = mod._cache
        if on_gpu:  # the optimiser pass writes the fp16 copies the forward kernels read (no cast pass per parameter and step)
            self.opt.half_caches = {p: c for p, c in self._cache_of.items() if p.numel() > 0}

    def _render(self, rays_o, rays_d, time, **kw):
        """model.render on `ray_chunks` slices of the batch, results concatenated.  Each slice is its own autograd sub-graph, and
        backward walks them one after the other (last slice first), so the table scatter of a slice (side stream) runs beside the
        backward of the next slice, and the activations of one slice at a time are alive (peak memory 1.9 -> 1.4 GiB at 4
        slices).  Measured on one MI355X it does NOT shorten the step (10.6 ms at 1 slice, 10.9 at 2, 12.7 at 4): the scatter
        saturates the memory-side atomic path -- read-modify-write of a 64-B segment per 8-16 useful bytes, about 5 TB/s of
        HBM traffic -- and whatever runs beside it is slowed by what it gains.  Default 1; a memory knob, not a speed knob.
        Per-ray results do not depend on the slicing; only the order in which the fp32 table gradients are added changes."""
        N = rays_o.shape[1]
        k = min(self.ray_chunks, max(1, N // 256))
        if k <= 1:
            return self.model.render(rays_o, rays_d, time, **kw)
        cuts = [N * i // k for i in range(k + 1)]
        outs = [self.model.render(rays_o[:, a:b], rays_d[:, a:b], time, **kw) for a, b in zip(cuts[:-1], cuts[1:])]
        merged = {}
        for key, v in outs[0].items():
            if not torch.is_tensor(v):
                merged[key] = v
                continue
            dim = 1 if (v.dim() >= 2 and v.shape[0] == 1 and v.shape[1] == cuts[1] - cuts[0]) else 0
            merged[key] = torch.cat([o[key] for o in outs], dim=dim)
        return merged

    def _distortion(self, r, rays_o, rays_d, lidar):
        """The distortion term on the rows of the render `r` of the rays (rays_o, rays_d) [1, N, 3]; nears and fars as `run` forms them."""
        m = self.model
        o, d = rays_o.contiguous().view(-1, 3).float(), rays_d.contiguous().view(-1, 3).float()
        nears, fars = m._near_far(o, d, lidar, m.aabb_train if m.training else m.aabb_infer)
        term = DistortionLossFn.apply if r["weights"].is_cuda else distortion_loss_host
        return term(r["weights"], r["z_vals"], nears, fars, self.alpha_dist)

    def _chamfer(self, a, b):
        if self._cham is None:
            from nvsf.nerf.chamfer3D.dist_chamfer_3D import chamfer_3DDist
            self._cham = chamfer_3DDist()
        return self._cham(a, b)

    def flow_loss(self, time):
        """Scene-flow loss of trainer.py:236-267: the frame's point cloud moved by the predicted forward / backward flow against
        the next / previous frame's cloud (sum of squared NN distances both ways, x 0.5) + the mean absolute flow."""
        frame_idx = int(float(time.reshape(-1)[0]) * (self.model.num_frames - 1))
        pc = self.pc_list.get(frame_idx)
        if pc is None:
            return None
        pc = pc.float().contiguous()
        pred = self.model.flow(pc, time)
        total = None
        for key, other in (("flow_forward", frame_idx + 1), ("flow_backward", frame_idx - 1)):
            tgt = self.pc_list.get(other)
            if tgt is None:
                continue
            d1, d2, _, _ = self._chamfer((pc + pred[key]).unsqueeze(0), tgt.float().contiguous().unsqueeze(0))
            term = (d1.sum() + d2.sum()) * 0.5 + pred[key].abs().mean()
            total = term if total is None else total + term
        return total

    def losses(self, batch):
        """batch: rays_o_lidar, rays_d_lidar [1,N,3] with either images_lidar [1,N,3] = (raydrop, intensity, range) as the
        reference's loader delivers them or gt_raydrop / gt_intensity / gt_depth [1,N]; rays_o, rays_d [1,N,3] with gt_rgb
        (or images) [1,N,3]; time [1,1].  Returns (total, parts)."""
        m, out = self.model, {}
        if "rays_o_lidar" in batch:
            if "images_lidar" in batch:
                gt_rd, gt_i, gt_d = (batch["images_lidar"][:, :, k] for k in range(3))
            else:
                gt_rd, gt_i, gt_d = batch["gt_raydrop"], batch["gt_intensity"], batch["gt_depth"]
            r = self._render(batch["rays_o_lidar"], batch["rays_d_lidar"], batch["time"], cal_lidar_color=True, perturb=True,
                             num_steps=self.num_steps, **self._resample_kw)
            on_device = r["depth_lidar"].is_cuda
            pH, pW = self._patch_dims()
            if pH > 1 and self.grad_loss and not on_device:
                raise NotImplementedError("grad_loss (the structural regulariser on LiDAR patches) exists as HIP kernels only: the host branch would drop the 'sr' term silently")
            # device: one HIP launch each way for the three sums, the masked range and the chamfer point clouds; host-side logic tests:
            # the same terms as torch expressions
            # (non-default criteria: the `_crit` pair / the torch.nn criteria, one argument more)
            if self.lidar_criteria is None:
                lidar_terms, crit = (LidarLossFn.apply if on_device else lidar_losses_host), ()
            else:
                lidar_terms, crit = (LidarCritLossFn.apply if on_device else lidar_losses_host), (self.lidar_criteria,)
            d = batch["rays_d_lidar"] if self.use_chamfer else None
            out["depth"], out["raydrop"], out["intensity"], pred_depth, pred_pts, gt_pts = lidar_terms(
                r["image_lidar"], r["depth_lidar"], gt_rd, gt_i, gt_d, d, self.alpha_d, self.alpha_r, self.alpha_i, self.smooth, self.scale, *crit)
            if self.use_chamfer:
                d1, d2, _, _ = self._chamfer(pred_pts, gt_pts)
                out["chamfer"] = (d1 + d2).mean() * 0.5
            if pH > 1 and self.grad_loss:
                if "rays_pano_inds" not in batch or "pano_frame" not in batch:
                    raise ValueError("grad_loss on LiDAR patches needs batch['rays_pano_inds'] and batch['pano_frame'] (FrameSet.train_batch)")
                out["sr"] = LidarGradLossFn.apply(pred_depth, gt_d * gt_rd, gt_rd, batch["rays_pano_inds"], batch["pano_frame"], (pH, pW),
                                                  self.scale, self.depth_grad_loss, self.alpha_grad, self.sobel_grad)
            if self.error_maps is not None and on_device:
                self._for_error_map["lidar"] = (r["image_lidar"].detach(), r["depth_lidar"].detach(), gt_rd, gt_i, gt_d)
            if self.use_flow:
                fl = self.flow_loss(batch["time"])
                if fl is not None:
                    out["flow"] = fl
            if self.use_urf:
                eps = 0.02 * 0.1 ** min(self.global_step / self.iters, 1)
                # device: two streaming passes forward, one backward (UrfLossFn); host-side logic tests: the torch expression
                out["los"] = (UrfLossFn.apply if on_device else urf_line_of_sight_loss)(r["weights"], r["z_vals"], gt_d * gt_rd, eps)
            if self.distortion:
                out["dist_lidar"] = self._distortion(r, batch["rays_o_lidar"], batch["rays_d_lidar"], True)
        if "rays_o" in batch:
            gt_rgb = batch["gt_rgb"] if "gt_rgb" in batch else batch["images"][..., :3]
            r = self._render(batch["rays_o"], batch["rays_d"], batch["time"], perturb=True, num_steps=self.num_steps, bg_color=1,
                             **self._resample_kw)
            if not self.use_rgbd_loss:
                if not r["image"].is_cuda:
                    out["rgb"] = rgb_loss_host(r["image"], gt_rgb, self.alpha_rgb, self.criteria["rgb_loss"], self.scale)
                elif self.rgb_criterion is None:
                    out["rgb"] = MseSumFn.apply(r["image"], gt_rgb, self.alpha_rgb)
                else:
                    out["rgb"] = CritSumFn.apply(r["image"], gt_rgb, self.alpha_rgb, self.rgb_criterion, self.scale)
            else:
                if "gt_rgb_depth" not in batch:
                    raise ValueError("use_rgbd_loss needs batch['gt_rgb_depth'] (FrameSet(camera_depth=True).train_batch)")
                gt_m = batch["gt_rgb_depth"].reshape(r["depth"].shape)
                if r["image"].is_cuda:  # both camera terms in one HIP launch each way
                    camera_terms, crit = (CameraLossFn.apply, ()) if self.rgb_criterion is None else (CameraCritLossFn.apply, (self.rgb_criterion,))
                    out["rgb"], out["rgb_depth"] = camera_terms(r["image"], r["depth"], gt_rgb, gt_m, self.alpha_rgb, self.alpha_rd, self.scale,
                                                                self.rgb_depth_loss, *crit)
                else:  # host-side logic tests: the same terms as torch expressions
                    out["rgb"] = rgb_loss_host(r["image"], gt_rgb, self.alpha_rgb, self.criteria["rgb_loss"], self.scale)
                    out["rgb_depth"] = rgb_depth_loss_host(r["depth"], gt_m, self.scale, self.rgb_depth_loss, self.alpha_rd)
            if self.distortion:
                out["dist"] = self._distortion(r, batch["rays_o"], batch["rays_d"], False)
            if self.error_maps is not None and r["image"].is_cuda:
                self._for_error_map["camera"] = (r["image"].detach(), gt_rgb)
        total = sum(out.values())
        total = torch.nan_to_num(total, nan=0.0, posinf=1e5, neginf=1e5)  # trainer.py:545-546 (|inf| -> 1e5)
        return total, out

    def _patch_dims(self):
        p = self.patch_size_lidar
        if isinstance(p, int):
            return p, p
        return (p[0], p[0]) if len(p) == 1 else (p[0], p[1])

    def set_epoch(self, epoch, frames=None):
        """The per-epoch switch of trainer.py:1035-1062: with change_patch_size_lidar[0] > 1, every change_patch_size_epoch-th epoch
        samples LiDAR PATCHES (and regularises on them; the sampler draws from the error map when use_error_map), the others random
        pixels.  `frames`: the FrameSet whose sampler follows (default: the one given to attach_error_maps)."""
        frames = frames if frames is not None else self.error_maps
        if self.change_patch_size_lidar[0] > 1:
            patch = epoch % self.change_patch_size_epoch == 0
            self.pixel_sampler = "patch" if patch else "random"
            self.patch_size_lidar = tuple(self.change_patch_size_lidar) if patch else 1
            if frames is not None:
                frames.patch_size_lidar = self.patch_size_lidar
        if frames is not None:
            frames.use_error_map = self.use_error_map and self.pixel_sampler != "random"
        return self.pixel_sampler

    def attach_error_maps(self, frames):
        """`frames`: a FrameSet with enable_error_maps() called -- after every step the per-ray losses of the batch are written into
        its error_map / error_map_rgb (update_error_maps), as Trainer.train_step does whatever the sampler (trainer.py:552-630)."""
        if getattr(frames, "error_map", None) is None:
            frames.enable_error_maps()
        self.error_maps = frames

    def update_error_maps(self, batch):
        """trainer.py:552-630: the per-ray losses of the batch `losses` stashed go into the error maps of the batch's frame, per modality
        (losses.update_error_map)."""
        frames, stash = self.error_maps, self._for_error_map
        self._for_error_map = {}
        if frames is None or "index" not in batch:
            return
        idx = int(batch["index"][0])
        rgb = None if self.rgb_criterion is None else (self.rgb_criterion,)
        for key, inds_key, alphas, criteria in (("lidar", "rays_pano_inds", (self.alpha_d, self.alpha_r, self.alpha_i), self.lidar_criteria),
                                                ("camera", "rays_rgb_inds", (self.alpha_rgb,), rgb)):
            if key in stash and inds_key in batch:
                update_error_map(frames, idx, key, stash[key], batch[inds_key], alphas, self.smooth, criteria, self.scale)

    CAMERA_KEYS = ("rays_o", "rays_d", "gt_rgb", "images", "rays_rgb_inds", "H", "W", "gt_rgb_depth")

    def _backward(self, loss):
        overlap = loss.is_cuda and self.scatter_overlap
        local_sink = False
        tctx = self.train_ctx
        if overlap:
            from nvsf import field_ops
            tctx.overlap = True
            if tctx.sink is None:  # one process: the side-stream scatters accumulate straight into p.grad
                if self._sink is None:
                    self._sink = field_ops.LocalGradSink()
                tctx.sink, local_sink = self._sink, True
        try:
            self.scaler.scale(loss).backward()
            tctx.end_pass()  # a table announced but not scattered into as often is marked ready behind what it received
        finally:
            if overlap:
                tctx.overlap = False
                if local_sink:
                    tctx.sink = None
        return overlap

    def sync(self):
        """The calling stream waits for the optimiser pass `step` left on the scatter stream (the last table's).  Readers inside this
        package that go through the encoders' fp16 copies wait by themselves (tinycudann._HalfCache.pending); call this before
        touching the fp32 parameters or the optimiser state directly (end_epoch / checkpoint_state / load_checkpoint do)."""
        if self._late_carry is not None:
            # a late-only overflow that has not reached the scaler yet is settled here (callers: end of epoch, checkpoint, load -- the
            # host is waiting anyway), so that it is neither lost with a checkpoint nor applied to a freshly loaded scaler
            ev_c, carry = self._late_carry
            self._late_carry = None
            ev_c.synchronize()
            self.scaler.release_growth(carry)
            if float(carry) != 0.0:
                self.scaler.update(carry)
        if self._pending is not None:
            ev, params = self._pending
            torch.cuda.current_stream().wait_event(ev)
            self._mark_pending(params, None, match=ev)
            self._pending = None

    def _mark_pending(self, params, ev, match=None):
        """Sets the pending event of the fp16 cache and of the K-planes owner (read as fp32 by its kernels: the module makes its first
        reader wait) of each late parameter to `ev`; ev None clears it where it is still `match`."""
        for p in params:
            cache = self._cache_of.get(p)
            if cache is not None and (ev is not None or cache.pending is match):
                cache.pending = ev
            owner = self._plane_owner.get(p)
            if owner is not None and (ev is not None or owner.__dict__.get("_pending_update") is match):
                owner.__dict__["_pending_update"] = ev

    def _late_step(self, late):
        """The optimiser pass of a step whose last table scatters (`late`: [(parameter, scatter event)]) are still running on the side
        stream.  -> (found, carry, ev): the overflow flag of the early gradients (None without loss scaling), the late-only overflow
        for `_late_carry` (None likewise), the event behind the late tables' pass."""
        # every gradient but the late tables' is final on this stream: the step's overflow decision is taken from those (for a
        # table fed by an fp32 input gradient that is sufficient: loss_scaler.py), their update here, the late tables' update
        # behind their scatter on the side stream.  A table fed through an fp16 hand-over (the static hash of the space-time
        # field: the density tail's gradient-split kernel casts a finite fp32 dX > 65504 to inf) is NOT covered by that argument,
        # so the late gradients are inspected as well -- on the side stream, behind their scatter: `found_late` = early OR late
        # is what the late tables' Adam pass skips on (no inf / nan can reach a table, its EMA shadow or its fp16 copy), and an
        # overflow seen ONLY there reaches the scaler's update one step later (`_late_carry`: the scale is halved after the next
        # step instead of this one; waiting for it here would put the scatter back on the critical path).
        from nvsf import field_ops
        late_set = {p for p, _ in late}
        early = [p for g in self.opt.param_groups for p in g["params"] if p.grad is not None and p not in late_set]
        if self.scaler.is_enabled():
            found = self.scaler.found_inf([p.grad for p in early])
            scale = self.scaler.scale_tensor()
            self.opt.grad_scale, self.opt.found_inf = scale, found
        else:
            found = None
        carry = None
        try:
            self.opt.step(params=early)
            main = torch.cuda.current_stream()
            side = field_ops.side_stream(late[0][0].device)
            side.wait_stream(main)  # found / scale exist; (the scatters themselves are already in front of us on `side`)
            with torch.cuda.stream(side):
                for p in late_set:
                    p.grad.record_stream(side)  # zero_grad of the next step drops the tensor while this pass may still read it
                if found is not None:
                    found.record_stream(side)
                    scale.record_stream(side)
                    late_only = self.scaler.found_inf([p.grad for p in late_set])
                    self.opt.found_inf = torch.maximum(found, late_only)
                    carry = torch.clamp_(late_only - found, min=0.0)  # 1 only when the early gradients were clean
                self.opt.step(params=list(late_set))
                ev = torch.cuda.Event()
                ev.record(side)
        finally:
            if found is not None:
                del self.opt.grad_scale, self.opt.found_inf
        self._pending = (ev, list(late_set))
        self._mark_pending(late_set, ev)
        return found, carry, ev

    def step(self, batch):
        defer = self.defer_last_table and self.scatter_overlap
        loss, parts, n_coll, late = self._run(batch, defer)
        if getattr(self.model, "cuda_ray", False):
            from nvsf.nerf.raymarching import raymarching
            if raymarching.march_status_pending():  # occupancy-grid training without a counter read-back: the marcher's failure flag
                raymarching.check_march_status(wait=True)  # is looked at before the optimiser, not one call later
        found, carry, ev = self._late_step(late) if late else (self.scaler.step(self.opt), None, None)
        if found is not None:
            prev, self._late_carry = self._late_carry, (None if carry is None else (ev, carry))
            if prev is not None:  # a late-only overflow of the PREVIOUS step (its event is long past: this step's passes read that table)
                main = torch.cuda.current_stream()
                main.wait_event(prev[0])
                prev[1].record_stream(main)  # allocated on the side stream, consumed here
                self.scaler.release_growth(prev[1])  # the doubling the previous step earned, unless its late check found an overflow
                found = torch.maximum(found, prev[1])
            # this step's late check still pending: its `found` may yet turn out to have been an overflow, so a growth interval it
            # completes doubles the scale only at the next step, once that check is known (else the scale would double now and halve
            # one step later); the tracker itself advances as GradScaler's does
            self.scaler.update(found, hold=self._late_carry is not None)
        if self.error_maps is not None:
            self.update_error_maps(batch)
        self.sched.step()
        self.global_step += 1
        return loss, parts, n_coll

    def forward_backward(self, batch):
        """Everything of a step up to (not including) the optimiser: both renders, the losses, backward through the HIP operators,
        the gradient all-reduce when there is more than one rank; on return every parameter's `.grad` (still multiplied by the
        loss scale) is final on the current stream.  -> (loss, parts, number of collectives).  `step` = this + Adam (with the
        wait for the last table scatter moved behind the optimiser pass of everything else)."""
        return self._run(batch, False)[:3]

    def _run(self, batch, defer):
        if self.model.__dict__.get("_train_ctx") is not self.train_ctx:  # another step object was built on this model since
            for mod in self.model.modules():
                mod.__dict__["_train_ctx"] = self.train_ctx
        self.train_ctx.begin_step()  # a table is final after the LAST scatter it receives in a backward pass (ray_chunks > 1: several)
        self._sink = None
        try:
            return self._forward_backward(batch, defer)
        finally:
            self.train_ctx.end_step()
            self._sink = None

    def _forward_backward(self, batch, defer=False):
        self.model.train()
        if self.buckets is not None:
            self.buckets.begin_step()
        else:
            self.opt.zero_grad(set_to_none=True)
        if self.split_backward and "rays_o_lidar" in batch and "rays_o" in batch:
            lidar = {k: v for k, v in batch.items() if k not in self.CAMERA_KEYS}
            camera = {k: v for k, v in batch.items() if k in self.CAMERA_KEYS or k == "time"}
            loss, parts, overlap = None, {}, False
            # Camera pass first: its table scatter is the longer one (2.85 against 2.07 ms at 4096 + 4096 rays x 768: camera samples
            # sit in cells of their own at the five finest levels) and, issued first, it runs on the side stream beside the whole
            # LiDAR pass (forward + backward, 2.7 ms); only the shorter LiDAR scatter is left exposed at the end of the step.
            for first, sub in ((True, camera), (False, lidar)):
                if self.buckets is not None:  # parameters both passes reach (the sigma MLP) are final only after the second
                    self.buckets.hold(first)
                part_loss, part = self.losses(sub)
                n_before = len(self._sink.side_scatters) if self._sink is not None else 0
                overlap = self._backward(part_loss) or overlap
                self._last_pass_tables = {p for p, _ in self._sink.side_scatters[n_before:]} if self._sink is not None else set()
                loss = part_loss.detach() if loss is None else loss + part_loss.detach()
                parts.update(part)
            if self.buckets is not None:
                self.buckets.release_held()
        else:
            loss, parts = self.losses(batch)
            overlap = self._backward(loss)
            self._last_pass_tables = set()  # one joint backward: nothing is left to overlap a deferred pass with -- all tables early
        # the all-reduce is linear: it runs on the scaled gradients (an inf / nan on one rank reaches every rank, so all of
        # them skip the step together); scaler.step unscales, checks and steps.  Buckets go out during backward (hooks); finish()
        # closes the rest, waits and averages.  The table scatters run on a side stream: their consumers wait here.
        late = []
        if self.buckets is not None:
            n_coll = self.buckets.finish()
        else:
            n_coll = 0
            if overlap:
                from nvsf import field_ops
                scatters = self._sink.side_scatters if self._sink is not None else []
                if defer and scatters:
                    # wait only for the tables scattered BEFORE the last backward pass (long finished); the last pass' tables stay late
                    last_pass = self._last_pass_tables
                    main = torch.cuda.current_stream()
                    for p, ev in scatters:
                        if p in last_pass:
                            late.append((p, ev))
                        else:
                            main.wait_event(ev)
                else:
                    field_ops.sync_side_streams()
        return loss.detach(), {k: v.detach() for k, v in parts.items()}, n_coll, late

    def end_epoch(self):
        """What the reference does after the step loop of an epoch (trainer.py:1420-1421): one EMA update."""
        self.sync()
        if self.ema is not None:
            self.ema.update()

    def checkpoint_state(self, epoch=0, stats=None, full=True, reference_layout=False, refiner=None):
        """The dict Trainer.save_checkpoint writes with torch.save (nvsf/nerf/utils.py:622-648): epoch, global_step, stats,
        model and -- for a `full` checkpoint -- optimizer, lr_scheduler, scaler, ema.  `model` always speaks the reference's
        schema (names and shapes).  `optimizer` and `ema` are lists by parameter position: written in this package's layout (one
        entry per `planes_cl`) unless `reference_layout`, which expands the optimiser entry to one state per plane so that a
        reference Trainer resumes from it (checkpoint_compat); the `ema` entry cannot be written for the reference -- torch_ema
        wants shadows for the three unused modules this model does not have -- and the reference then starts a fresh average,
        as it does for any checkpoint whose ema fails to load (utils.py:728-747).  load_checkpoint reads both layouts.
        `refiner`: a RaydropRefiner (nvsf/nerf/refine.py) whose `unet.*` entries join `model`, which is what the reference saves after
        its refinement (trainer.py:1011-1012); RaydropRefiner.load_from_checkpoint reads them back."""
        self.sync()
        state = {"epoch": epoch, "global_step": self.global_step, "stats": stats if stats is not None else {}}
        if full:
            state["optimizer"] = self.opt.state_dict()
            if reference_layout:
                from nvsf.nerf import checkpoint_compat as compat
                state["optimizer"] = compat.optimizer_state_in_reference_layout(state["optimizer"], self.model, self.opt)
            state["lr_scheduler"] = self.sched.state_dict()
            state["scaler"] = self.scaler.state_dict()
            if self.ema is not None:
                state["ema"] = self.ema.state_dict()
        state["model"] = self.model.state_dict()
        if refiner is not None:
            state["model"].update(refiner.state_entries())
        return state

    def save_checkpoint(self, path, epoch=0, stats=None, full=True, reference_layout=False, refiner=None):
        torch.save(self.checkpoint_state(epoch, stats, full, reference_layout, refiner), path)

    def load_checkpoint(self, checkpoint, model_only=False):
        """Trainer.load_checkpoint (nvsf/nerf/utils.py:682-747): a bare state_dict loads strictly; a checkpoint dict loads its
        model with strict=False (the reference's files carry three unused sub-modules), then global_step / optimizer /
        lr_scheduler / scaler / ema where present.  checkpoint: path or the loaded dict.  Returns (missing_keys, unexpected_keys,
        epoch); `self.failed_to_load` lists the components whose state could not be restored (each also raises a warning, as
        the reference logs "[WARN] Failed to load ..." and trains on, utils.py:728-747)."""
        self.sync()
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location=next(self.model.parameters()).device)
        if "model" not in checkpoint:
            self.model.load_state_dict(checkpoint)
            return [], [], None
        missing, unexpected = self.model.load_state_dict(checkpoint["model"], strict=False)
        self.failed_to_load = []

        from nvsf.nerf import checkpoint_compat as compat

        def translate(key, state):
            """`ema` / `optimizer` entries are ordered by parameter POSITION: a reference checkpoint counts three unused modules and
            24 tensors per Planes4D where this model has one (checkpoint_compat)."""
            if key == "ema":
                state = dict(state, shadow_params=compat.shadows_for_model(state["shadow_params"], self.model))
                if state.get("collected_params") is not None:
                    state["collected_params"] = compat.shadows_for_model(state["collected_params"], self.model)
            elif key == "optimizer":
                state = compat.optimizer_state_for_model(state, self.model, self.opt)
            return state

        def restore(key, obj):
            if key in checkpoint and obj is not None:
                try:
                    obj.load_state_dict(translate(key, checkpoint[key]))
                except Exception as e:  # noqa: BLE001 -- reference behaviour: warn and continue
                    self.failed_to_load.append(key)
                    warnings.warn(f"[WARN] Failed to load {key} state from the checkpoint ({type(e).__name__}: {e}); "
                                  f"continuing with a fresh {key}")
                    if key == "ema":
                        # "fresh" = the average starts again FROM THE WEIGHTS JUST LOADED: the shadows still hold the clones taken
                        # at construction (random init), which evaluate_frames(ema=...) would otherwise copy over the checkpoint
                        obj.reset_to_parameters()
        restore("ema", self.ema)  # before the model_only return, as the reference does (utils.py:715-719): evaluation runs under the EMA weights
        if model_only:
            return list(missing), list(unexpected), checkpoint.get("epoch")
        if "global_step" in checkpoint:
            self.global_step = checkpoint["global_step"]
        for key, obj in (("optimizer", self.opt), ("lr_scheduler", self.sched), ("scaler", self.scaler)):
            restore(key, obj)
        return list(missing), list(unexpected), checkpoint.get("epoch")
