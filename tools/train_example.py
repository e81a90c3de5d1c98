"""End-to-end example of the multimodal training loop around the hot path (BASELINE config 4), one process per GPU:

    python tools/train_example.py --root /path/to/kitti360_nvsf --sequence 1908 [--dynamic] [--epochs 6] [--plain]
                                  [--export-mesh out.ply --mesh-res 256 256 256 --mesh-threshold 10] [--dynamic --flow-loss]
                                  [--eval-table] [--rgbd-loss] [--depth-mode {mean,median,mode}] [--annotations boxes.json [--offset X Y Z]]
                                  [--refine [--refine-iterations N]]
                                  [--test-export DIR [--delta-position X Y Z] [--delta-orientation R P Y] [--lidar-channels V] [--lidar-columns N]
                                   [--intrinsics-lidar-new UP FOV] [--intrinsics-hoz-lidar-new UP FOV] [--delta-pos-camera X Y Z]
                                   [--delta-orient-camera R P Y] [--height-new H] [--width-new W]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 tools/train_example.py ...

Data: the reference's on-disk formats (transforms_{seq}_{split}.json + range-image .npy + images; nvsf/nerf/dataset/formats.py).
Without --root a small synthetic data set in those formats is written to a temporary directory first.
Every step renders one frame per rank (frames are sharded over the ranks, nvsf/frame_shard.py), then ONE bucketed RCCL
all-reduce of the gradients, then Adam under the loss scaler (nvsf/nerf/train_step.py).  The loop is the shipped configuration's
(configs/kitti360_1908.txt: grad_loss, use_error_map; trainer.py:1035-1062): epochs over the frames, every second epoch samples 2 x 8 LiDAR
patches from the error map and adds the structural regularisation, every step writes its per-ray losses back into the frame's error maps,
one EMA update per epoch; --plain = random pixels and the default losses only.  Reports loss terms, PSNR, range RMSE, CD / F-score.
--export-mesh then writes the density field's marching-cubes mesh (nvsf/nerf/mesh.py) at the time of the first evaluation frame.
--flow-loss (with --dynamic) builds the scene-flow point clouds from the range images before the first epoch (Trainer.process_pointcloud,
trainer.py:1848-1912; here nvsf/nerf/pointcloud.py on the device) and switches the flow term of the loss on.
--eval-table also prints the report lines of the reference's evaluation table (trainer.py:1794-1827): range and intensity RMSE / MedAE /
LPIPS / SSIM / PSNR, ray-drop RMSE / accuracy / F1, camera PSNR / RMSE / SSIM, computed on the device (nvsf/nerf/meters.py).
--rgbd-loss (the reference's --use_rgbd_loss, main_nvsf.py:84) projects every frame's range image into its camera once, on the device
(nvsf/nerf/dataset/depth_image.py), and supervises the camera render's depth with that map; with --eval-table the table gets the camera
depth RMSE line the reference prints as "RMSE = ".
--annotations PATH (with --eval-table): a JSON sidecar of the moving objects' 3-D boxes, {"<frame_id>": [{"class": str, "vertices":
[[x, y, z] x 8]}, ...]} in the world frame in metres (--offset: the recentring of the poses, the reference's --offset); the table is then
also printed over the static background and over the boxes (trainer.py:1545-1626; masks on the device, nvsf/nerf/object_masks.py).
--refine (the shipped configuration's use_refine): after training, the ray-drop refinement U-Net is fitted on the staged renders of the
training frames (Trainer.refine, trainer.py:905-1017; nvsf/nerf/refine.py, --refine-iterations steps, the reference's 1000) and the
evaluation is reported twice, without and with it, as the reference logs both; the refined evaluation runs the U-Net's HIP forward
(csrc/unet.hip) once per frame.
--test-export DIR (the reference's Trainer.test, trainer.py:1109-1283): after training, every frame of the split is rendered without
ground truth (evaluate.test_step) and written out as the simulated LiDAR sweep -- text clouds in the world and the LiDAR frame, a PCD
file -- and as PNGs of the ray-drop mask / intensity / range stack, the camera image and its depth (nvsf/nerf/export.py; clouds and
uint8 planes built on the device, csrc/export.hip).  The sensor flags (main_nvsf.py:121-131; base_dataset.py:168-227) render it from a
NOVEL sensor: the LiDAR moved by --delta-position (metres) / --delta-orientation (degrees), with --lidar-channels beams (the range image
gets two more rows) and --lidar-columns columns, other fields of view; the camera moved and resized likewise.  With --refine the
exported ray-drop plane is the U-Net's.
--mesh-normals (with --export-mesh) writes the unit normals -grad sigma / |grad sigma| of the density field with the mesh's vertices;
--normal-maps DIR writes, for each evaluation frame, normal_lidar_XXXX.png and normal_XXXX.png: the composited normals sum_i w_i n_i of
the LiDAR and the camera rays as (n + 1) / 2 in RGB (nvsf/nerf/normals.py).  Both work for either model: with --dynamic the gradient is
taken at each frame's time, through the space-time encoders and the flow warp.
--depth-mode median | mode: the evaluation (its range rows, chamfer distance and F-score) and the --test-export clouds
take a ray's range from the median of its termination distribution, resp. from its strongest return, instead of the mean sum w z that
floats between two surfaces at an object's edge (run(depth_mode=...): one HIP launch per ray batch on the rows the render returns).
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

import numpy as np
import torch


def synthetic_dataset(root, seq, n_frames=8, H=376, W=1408, Hl=66, Wl=1030, seed=0, street=False):  # KITTI-360's image / range-image sizes
    """A box-shaped toy scene in the reference's formats: constant-colour images, a range image of a sphere of radius 30 m.
    `street` (--flow-loss): the range images show a ground plane and boxes instead, one of which moves 1 m per frame."""
    from nvsf import synthetic as S
    from nvsf.nerf.dataset import formats as F
    rng = np.random.default_rng(seed)
    boxes = S.street_range_image(np.random.default_rng(seed), hw=(Hl, Wl))[1] if street else None
    d = os.path.join(root, "train", seq)
    os.makedirs(d, exist_ok=True)
    frames = []
    for i in range(n_frames):
        pose = np.eye(4)
        pose[:3, 3] = [0.2 * i, 0.0, 0.0]
        img = np.full((H, W, 3), 120 + 10 * i, np.uint8)
        pc = np.zeros((Hl, Wl, 3), np.float32)
        pc[..., 1] = rng.random((Hl, Wl)) * 0.5
        pc[..., 2] = 30.0
        pc[rng.random((Hl, Wl)) < 0.1, 2] = 0.0
        if street:
            moved = boxes.copy()
            moved[0, [0, 3]] += 1.0 * i
            pc[..., 2] = S.street_range_image(rng, boxes=moved, hw=(Hl, Wl))[0]
        np.save(os.path.join(d, f"img_{i:04d}.npy"), img)
        np.save(os.path.join(d, f"pano_{i:04d}.npy"), pc)
        frames.append({"frame_id": 1908 + i, "file_path": f"train/{seq}/img_{i:04d}.npy", "transform_matrix": pose,
                       "lidar_file_path": f"train/{seq}/pano_{i:04d}.npy", "lidar2world": pose})
    K = np.array([[552.55, 0, W / 2], [0, 552.55, H / 2], [0, 0, 1]])
    F.write_transforms(F.transforms_path(root, seq, "train"), w=W, h=H, w_lidar=Wl, h_lidar=Hl, K=K, frame_start=1908, frame_end=1908 + n_frames - 1,
                       num_frames=n_frames, frames=frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None)
    ap.add_argument("--sequence", default="1908")
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--plain", action="store_true", help="no structural regularisation / error maps / patch epochs")
    ap.add_argument("--num-rays", type=int, default=4096)
    ap.add_argument("--num-steps", type=int, default=768)
    ap.add_argument("--upsample-steps", type=int, default=0, metavar="U", help="hierarchical importance resampling: U more samples per ray drawn "
                    "from the coarse weights (RenderTrainStep(upsample_steps=U), run(hierarchical=True)); training, --eval-table and --test-export")
    ap.add_argument("--dynamic", action="store_true", help="the reference's space-time model instead of the static hash field")
    ap.add_argument("--flow-loss", action="store_true", help="scene-flow supervision of the space-time model (needs --dynamic): the frames' "
                    "LiDAR clouds are cleaned on the device first (nvsf/nerf/pointcloud.py)")
    ap.add_argument("--export-mesh", default=None, metavar="PATH", help="after training, write the density field's mesh as a binary PLY "
                    "(marching cubes on the device, at the time of the first evaluation frame; nvsf/nerf/mesh.py)")
    ap.add_argument("--mesh-res", type=int, nargs=3, default=[256, 256, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--mesh-threshold", type=float, default=10.0, help="density at the surface (inside: sigma >= threshold)")
    ap.add_argument("--mesh-normals", action="store_true", help="write vertex normals (-grad sigma / |grad sigma|) with --export-mesh (with --dynamic: at the mesh's frame time)")
    ap.add_argument("--normal-maps", default=None, metavar="DIR", help="after training, write normal_lidar_XXXX.png / normal_XXXX.png of every "
                    "evaluation frame: the rendered normals as (n + 1) / 2 (nvsf/nerf/normals.py; with --dynamic: at each frame's time)")
    ap.add_argument("--eval-table", action="store_true", help="after training, print the report lines of the reference's evaluation table "
                    "(device-side meters, nvsf/nerf/meters.py)")
    ap.add_argument("--depth-mode", default="mean", choices=["mean", "median", "mode"], help="the range --eval-table and --test-export report per ray: "
                    "the mean sum w z, the median of the termination distribution or the strongest return (run(depth_mode=...))")
    ap.add_argument("--rgbd-loss", action="store_true", help="camera depth supervision from the LiDAR-projected depth map (FrameSet(camera_depth=True), "
                    "RenderTrainStep(use_rgbd_loss=True)); adds the camera depth RMSE to --eval-table")
    for option, default in (("depth", "l1"), ("raydrop", "mse"), ("intensity", "mse"), ("rgb", "mse")):
        ap.add_argument(f"--{option}-loss", default=default, choices=["l1", "mse", "huber", "smoothl1", "bce"],
                        help=f"criterion of the {option} term (RenderTrainStep({option}_loss=...))")
    ap.add_argument("--urf-loss", action="store_true", help="line-of-sight loss of Urban Radiance Fields on the LiDAR samples "
                    "(RenderTrainStep(use_urf_loss=True): one HIP pass each way)")
    ap.add_argument("--distortion-loss", action="store_true", help="distortion loss of mip-NeRF 360 on the samples of both renders "
                    "(RenderTrainStep(distortion_loss=True): parts dist_lidar and dist, one HIP scan per ray each way)")
    ap.add_argument("--alpha-dist", type=float, default=0.01, metavar="X", help="weight of the distortion loss")
    ap.add_argument("--annotations", default=None, metavar="PATH", help="JSON sidecar of the moving objects' 3-D boxes per frame id (world frame, "
                    "metres); --eval-table then also prints the static / dynamic tables (nvsf/nerf/object_masks.py)")
    ap.add_argument("--refine", action="store_true", help="fit the ray-drop refinement U-Net after training and evaluate with it as well "
                    "(nvsf/nerf/refine.py; HIP forward csrc/unet.hip)")
    ap.add_argument("--refine-iterations", type=int, default=1000, help="optimisation steps of the U-Net fit (the reference's 1000)")
    ap.add_argument("--test-export", default=None, metavar="DIR", help="after training, render every frame without ground truth and write the "
                    "predicted point clouds (world / LiDAR frame .txt, .pcd) and PNGs there (nvsf/nerf/export.py)")
    ap.add_argument("--delta-position", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"), help="move the LiDAR, metres, its own frame")
    ap.add_argument("--delta-orientation", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("R", "P", "Y"), help="turn the LiDAR, degrees")
    ap.add_argument("--lidar-channels", type=int, default=0, metavar="V", help="vertical channels of the new LiDAR (0: unchanged)")
    ap.add_argument("--lidar-columns", type=int, default=0, metavar="N", help="columns of the new range image (0: unchanged)")
    ap.add_argument("--intrinsics-lidar-new", type=float, nargs=2, default=[0.0, 0.0], metavar=("UP", "FOV"), help="new vertical field of view, degrees")
    ap.add_argument("--intrinsics-hoz-lidar-new", type=float, nargs=2, default=[0.0, 0.0], metavar=("UP", "FOV"), help="new horizontal field of view")
    ap.add_argument("--delta-pos-camera", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"), help="move the camera (front, left, up), metres")
    ap.add_argument("--delta-orient-camera", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("R", "P", "Y"), help="turn the camera, degrees")
    ap.add_argument("--height-new", type=int, default=0, metavar="H", help="height of the new camera image (0: unchanged)")
    ap.add_argument("--width-new", type=int, default=0, metavar="W", help="width of the new camera image (0: unchanged)")
    ap.add_argument("--offset", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"), help="world = pose / scale + offset")
    args = ap.parse_args()
    if args.annotations and not args.eval_table:
        ap.error("--annotations splits the evaluation table: add --eval-table")
    if args.flow_loss and not args.dynamic:
        ap.error("--flow-loss supervises the flow head of the space-time model: add --dynamic")
    if args.mesh_normals and not args.export_mesh:
        ap.error("--mesh-normals adds normals to the exported mesh: add --export-mesh PATH")
    from nvsf.nerf.dataset.formats import SensorChange
    sensor = SensorChange(delta_position=tuple(args.delta_position), delta_orientation=tuple(args.delta_orientation), H_lidar_new=args.lidar_channels,
                          W_lidar_new=args.lidar_columns, intrinsics_lidar_new=tuple(args.intrinsics_lidar_new),
                          intrinsics_hoz_lidar_new=tuple(args.intrinsics_hoz_lidar_new), delta_pos_camera=tuple(args.delta_pos_camera),
                          delta_orient_camera=tuple(args.delta_orient_camera), H_new=args.height_new, W_new=args.width_new)
    if not sensor.is_trivial() and not args.test_export:
        ap.error("the sensor flags change the sensors of the exported test render: add --test-export DIR")
    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    from nvsf import frame_shard, synthetic as S
    from nvsf.nerf.dataset.formats import FrameSet
    from nvsf.nerf.train_step import RenderTrainStep
    root = args.root
    if root is None:
        root = os.path.join(tempfile.gettempdir(), "nvsf_synthetic_street_376x1408" if args.flow_loss else "nvsf_synthetic_376x1408")
        if rank == 0:
            synthetic_dataset(root, args.sequence, street=args.flow_loss)
        if world > 1:
            dist.barrier()
    scale = S.SCALE if hasattr(S, "SCALE") else 0.010851959895748291
    data = FrameSet(root, args.sequence, "train", scale, num_rays=args.num_rays, num_rays_lidar=args.num_rays, device=dev,
                    camera_depth=args.rgbd_loss)
    torch.manual_seed(0)  # identical initial replicas
    if args.dynamic:
        from nvsf.nerf.models.network_dynamic import NeRFNetwork
        model = NeRFNetwork(time_resolution=8, num_frames=data.meta["num_frames"], bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR,
                            lidar_max_depth=S.LIDAR_MAX_DEPTH).to(dev)
    else:
        from nvsf.nerf.models.network_static import NeRFNetworkStatic
        model = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH,
                                  num_frames=data.meta["num_frames"]).to(dev)
    n = len(data)
    per_epoch = max(1, n // world)
    pc_list = None
    if args.flow_loss:  # every rank builds every frame's cloud: a step on frame k needs the clouds of k - 1 and k + 1
        import time
        from nvsf.nerf.pointcloud import process_pointcloud
        t0 = time.perf_counter()
        pc_list, pc_ground = process_pointcloud(FrameSet(root, args.sequence, "train", scale, device=dev, training=False), S.LIDAR_MAX_DEPTH)
        torch.cuda.synchronize()
        if rank == 0:
            print(f"scene-flow point clouds of {len(pc_list)} frames in {time.perf_counter() - t0:.2f} s: "
                  + "  ".join(f"{k}: {pc_list[k].shape[0]} points / {pc_ground[k].shape[0]} ground" for k in sorted(pc_list)), flush=True)
    trainer = RenderTrainStep(model, iters=args.epochs * per_epoch, num_steps=args.num_steps, scale=scale, grad_loss=not args.plain,
                              use_error_map=not args.plain, change_patch_size_lidar=(1,) if args.plain else (2, 8),
                              flow_loss=args.flow_loss, pc_list=pc_list, use_rgbd_loss=args.rgbd_loss, use_urf_loss=args.urf_loss,
                              depth_loss=args.depth_loss, raydrop_loss=args.raydrop_loss, intensity_loss=args.intensity_loss,
                              rgb_loss=args.rgb_loss, upsample_steps=args.upsample_steps, distortion_loss=args.distortion_loss,
                              alpha_dist=args.alpha_dist)
    render_kw = {"hierarchical": True, "upsample_steps": args.upsample_steps} if args.upsample_steps > 0 else {}
    if args.depth_mode != "mean":  # evaluation and export only: the training step supervises the mean
        if getattr(model, "cuda_ray", False):
            ap.error("--depth-mode reads the [N, T] rows of the uniform render, which the occupancy-grid path does not return")
        render_kw["depth_mode"] = args.depth_mode
    if not args.plain:
        trainer.attach_error_maps(data)
    it = 0
    for epoch in range(1, args.epochs + 1):
        sampler = trainer.set_epoch(epoch, data)  # "random" / "patch" (trainer.py:1035-1062)
        perm = np.random.default_rng(epoch).permutation(n)  # the same permutation on every rank
        sums, count = {}, 0
        for k in range(per_epoch):
            frame = int(perm[(k * world + rank) % n])
            loss, parts, n_coll = trainer.step(data.train_batch([frame]))
            for name, v in dict(parts, total=loss).items():
                sums[name] = sums.get(name, 0.0) + float(v)
            count += 1
            it += 1
        trainer.end_epoch()  # one EMA update per epoch (trainer.py:1420-1421)
        if rank == 0:
            line = f"epoch {epoch:3d}  sampler {sampler:6s}  " + "  ".join(f"{k} {v / count:.4f}" for k, v in sums.items()) + f"  all-reduces/step {n_coll}"
            if data.error_map is not None:
                em = data.error_map
                line += f"  error map: {int((em != 1).sum())} of {em.numel()} cells touched, max {float(em.max()):.1f}"
            print(line, flush=True)
    # whole-frame evaluation (Trainer.eval_step / evaluate_one_epoch): every frame rendered with the staged loop, its rays split over the ranks
    from nvsf.nerf.evaluate import evaluate_frames
    whole = FrameSet(root, args.sequence, "train", scale, device=dev, training=False, camera_depth=args.rgbd_loss,
                     annotations=args.annotations, offset=args.offset)
    refiner = None
    if args.refine:  # every rank fits the same U-Net from the same seed on the same renders
        import time
        from nvsf.nerf.refine import RaydropRefiner
        torch.manual_seed(0)
        refiner = RaydropRefiner(dev)
        t0 = time.perf_counter()
        losses = refiner.fit(model, whole, args.num_steps, ema=trainer.ema, iterations=args.refine_iterations,
                             generator=torch.Generator().manual_seed(0))
        torch.cuda.synchronize()
        if rank == 0:
            print(f"ray-drop refinement: {len(losses)} iterations over {len(whole)} frames in {time.perf_counter() - t0:.1f} s, "
                  f"BCE {np.mean(losses[:5]):.4f} -> {np.mean(losses[-5:]):.4f}", flush=True)
    for label, r in ((("", None),) + ((("refined ", refiner),) if refiner is not None else ())):
        res = evaluate_frames(model, whole, args.num_steps, indices=range(min(len(whole), 4)), ema=trainer.ema,
                              meters="table" if args.eval_table else None, refiner=r, **render_kw)
        if rank == 0:
            print(f"{label}evaluation over {res['frames']} frames: loss {res['loss']:.4f}, PSNR {res['psnr']:.2f} dB, range RMSE "
                  f"{res['depth_rmse_m']:.2f} m, chamfer distance {res['chamfer_distance']:.3f}, F-score {res['f_score']:.3f}")
            if args.eval_table:
                from nvsf.nerf.meters import table_report
                print("\n".join(table_report(res)), flush=True)
    if args.test_export:  # every rank renders its share of each frame's rays; rank 0 writes
        import time
        from nvsf.nerf.export import export_frames
        novel = FrameSet(root, args.sequence, "train", scale, device=dev, training=False, offset=args.offset, sensor=sensor)
        t0 = time.perf_counter()
        counts = export_frames(model, novel, args.test_export, f"{args.sequence}_ep{args.epochs:04d}", args.num_steps, refiner=refiner, ema=trainer.ema,
                               write=(rank == 0), **render_kw)
        torch.cuda.synchronize()
        if rank == 0:
            what = "changed sensors" if novel.sensor is not None else "the recording's sensors"
            print(f"test export ({what}: range image {novel.H_lidar} x {novel.W_lidar}, camera {novel.H} x {novel.W}): {len(counts)} frames, "
                  f"{counts} points, in {time.perf_counter() - t0:.2f} s -> {args.test_export}", flush=True)
    if args.export_mesh and rank == 0:
        from nvsf.nerf.mesh import export_mesh_density
        t_first = float(whole.collate([0])["time"].reshape(-1)[0])
        v, f = export_mesh_density(model, args.export_mesh, xyz_res=args.mesh_res, threshold=args.mesh_threshold, time=t_first,
                                   normals=args.mesh_normals)[:2]
        print(f"mesh at time {t_first:.4f}: {len(v)} vertices, {len(f)} triangles{' with normals' if args.mesh_normals else ''} -> {args.export_mesh}")
    if args.normal_maps and rank == 0:
        from nvsf.nerf.export import quantize_u8, write_png
        from nvsf.nerf.normals import render_normals
        os.makedirs(args.normal_maps, exist_ok=True)
        was_training = model.training
        model.eval()
        n_frames = min(len(whole), 4)
        for i in range(n_frames):
            data = whole.collate([i])
            for lidar, stem, hw in ((True, "normal_lidar", ("H_lidar", "W_lidar")), (False, "normal", ("H", "W"))):
                sfx = "_lidar" if lidar else ""
                out = render_normals(model, data["rays_o" + sfx].reshape(-1, 3), data["rays_d" + sfx].reshape(-1, 3), cal_lidar_color=lidar,
                                     num_steps=args.num_steps, time=data["time"] if args.dynamic else None)
                plane = ((out["normal"] + 1) / 2).reshape(int(data[hw[0]]), int(data[hw[1]]), 3)
                write_png(os.path.join(args.normal_maps, f"{stem}_{i:04d}.png"), quantize_u8(plane).cpu().numpy())
        model.train(was_training)
        print(f"normal maps of {n_frames} frames -> {args.normal_maps}")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
