"""Frame-sharded data parallelism over the GPUs of one node (one process per GPU, torch.distributed).

Rays are independent and a training step of the reference is one frame's ray batch (batch_size = 1 frame,
/root/reference/nvsf/nerf/dataset/base_dataset.py:415-421), so the path shards without any data-path collective:

  * training : rank r of W takes frame perm[epoch][step * W + r] (the DistributedSampler semantics the reference
               gestures at with `loader.sampler.set_epoch`, trainer.py:1301-1302); the ONLY communication is one
               bucketed all-reduce (sum, / W) of the gradients per step -- RCCL over xGMI with backend "nccl";
  * rendering: a frame's rays are split into W contiguous chunks and the [N/W, .] outputs are all-gathered
               (what trainer.py:1511-1524 intended).

The reference's own multi-GPU path is vestigial (DDP wrap without init_process_group, SURVEY finding 5); this
module is new design.  Everything here is host logic on torch tensors and runs unchanged on the gloo backend
(tests/test_frame_shard_cpu.py, world size 2).
"""
import torch
import torch.distributed as dist


def world():
    return (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)


def frame_order(num_frames, epoch, seed=0):
    """Epoch permutation shared by all ranks (same generator seed everywhere)."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(epoch))
    return torch.randperm(int(num_frames), generator=g).tolist()


def frames_for_rank(num_frames, epoch, rank, world_size, seed=0, drop_last=False):
    """Frames of this rank for one epoch, in step order.  Without drop_last the order is padded by wrapping around so
    every rank runs the same number of steps (and enters the same number of all-reduces)."""
    order = frame_order(num_frames, epoch, seed)
    if drop_last:
        order = order[: len(order) // world_size * world_size]
    elif len(order) % world_size:
        order = order + order[: world_size - len(order) % world_size]
    return order[rank::world_size]


def ray_chunk(n_rays, rank, world_size):
    """[begin, end) of this rank's contiguous chunk of a frame's rays (sizes differ by at most one)."""
    base, extra = divmod(int(n_rays), int(world_size))
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


def gather_ray_outputs(local, n_rays):
    """All-gathers per-rank [n_local, ...] outputs (ragged by at most one row) back into [n_rays, ...]."""
    rank, ws = world()
    if ws == 1:
        return local
    sizes = [ray_chunk(n_rays, r, ws)[1] - ray_chunk(n_rays, r, ws)[0] for r in range(ws)]
    width = max(sizes)
    pad = torch.zeros((width,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    bufs = [torch.empty_like(pad) for _ in range(ws)]
    dist.all_gather(bufs, pad)
    return torch.cat([b[:s] for b, s in zip(bufs, sizes)], dim=0)


def render_sharded(model, rays_o, rays_d, time, cal_lidar_color=False, max_ray_batch=4096, **kwargs):
    """Evaluation render of ONE frame's rays [1, N, 3] split over the ranks: rank r renders the contiguous chunk
    `ray_chunk(N, r, W)` with the staged loop of `NeRFRenderer.render` (renderer_dynamic.py:286-316: chunks of
    max_ray_batch rays, depth / image kept) and the per-rank outputs are all-gathered, so every rank returns the
    whole frame -- what the reference's eval loop intended with its all_gather of predictions (trainer.py:1511-1524).
    No collective touches the per-sample data; with one rank this is `model.render(..., staged=True)`."""
    rank, ws = world()
    N = rays_o.shape[1]
    begin, end = ray_chunk(N, rank, ws)
    keys = ("depth_lidar", "image_lidar") if cal_lidar_color else ("depth", "image")
    part = model.render(rays_o[:, begin:end].contiguous(), rays_d[:, begin:end].contiguous(), time, cal_lidar_color=cal_lidar_color,
                        staged=True, max_ray_batch=max_ray_batch, **kwargs)
    return {k: gather_ray_outputs(part[k][0], N).unsqueeze(0) for k in keys}


def allreduce_sums(values, device=None):
    """Sums a short list of host scalars over the ranks with ONE all-reduce -- the statistics collective of the reference's
    evaluation loop (`dist.all_reduce(loss, op=SUM); loss /= world_size`, trainer.py:1506-1509; SURVEY 8e: the only collective
    besides the gradients worth keeping).  fp64 on the wire; returns floats; the identity with one rank."""
    rank, ws = world()
    if ws == 1:
        return [float(v) for v in values]
    t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=device if device is not None else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return [float(v) for v in t.tolist()]


def allreduce_gradients(params, bucket_bytes=64 << 20):
    """Averages the gradients of `params` over all ranks AFTER backward has finished, in as few, as large all-reduces as
    `bucket_bytes` allows (one-shot form; `GradBuckets` is the overlapped form the training step uses).  A parameter without a
    gradient on this rank contributes zeros; a parameter without a gradient on EVERY rank keeps `grad = None`, so the optimiser
    skips it exactly as a single process would."""
    rank, ws = world()
    params = [p for p in params if p.requires_grad]
    if ws == 1 or not params:
        return 0
    gb = GradBuckets(params, bucket_bytes, hooks=False)
    had = [p.grad for p in params]
    gb.begin_step()
    for p, g in zip(params, had):
        if g is not None:
            p.grad.copy_(g)
            gb.mark_ready(p)
    return gb.finish()


class GradBuckets:
    """Gradient storage of a frame-sharded training step and its ONE collective per bucket, overlapped with backward.

    * Every bucket is one flat fp32 tensor; `p.grad` of its parameters are views into it (set by `begin_step`, which also zeroes
      the buckets), so autograd accumulates in place and a bucket is all-reduced as it stands -- no `torch.cat` / `.float()`
      staging copies of 190-375 MB of gradients after backward.
    * Buckets follow the order in which gradients become final in backward (the reverse of the order the parameters are
      given in, which is the order `get_params` lists them: tables first, heads last), so the heads' bucket is reduced while
      the table gradients are still being scattered.  A post-accumulate-grad hook counts a bucket's parameters; the last one
      launches `all_reduce(bucket, async_op=True)` -- RCCL over xGMI on a GPU node.  xGMI is point-to-point (7 links x ~153
      GB/s per GPU): ring time is set by the per-link rate, so buckets are few and large (64 MiB; a 49 MB table is its own).
    * `finish()` launches what has not been launched (parameters unused on this rank), reduces the per-parameter "somebody
      produced a gradient" flags, waits, averages, and sets `p.grad = None` for parameters no rank touched -- Adam then skips
      them, exactly as in a single process (a zero gradient would still move them by their momentum)."""

    def __init__(self, params, bucket_bytes=64 << 20, hooks=True, train_ctx=None):
        self.train_ctx = train_ctx  # field_ops.TrainContext of the step that owns these buckets (None: no kernel scatters into them)
        self.params = [p for p in params if p.requires_grad]
        self.ws = world()[1]
        order = list(reversed(self.params))
        self.buckets, cur, size = [], [], 0
        for p in order:
            nbytes = p.numel() * 4
            if cur and size + nbytes > bucket_bytes:
                self.buckets.append(cur)
                cur, size = [], 0
            cur.append(p)
            size += nbytes
        if cur:
            self.buckets.append(cur)
        self.flat, self.views, self.bucket_of = [], {}, {}
        for b, ps in enumerate(self.buckets):
            flat = torch.zeros(sum(p.numel() for p in ps), dtype=torch.float32, device=ps[0].device)
            off = 0
            for p in ps:
                if p.dtype != torch.float32:
                    raise TypeError("GradBuckets: fp32 parameters")
                self.views[p] = flat[off:off + p.numel()].view_as(p)
                self.bucket_of[p] = b
                off += p.numel()
            self.flat.append(flat)
        self._index = {p: i for i, p in enumerate(self.params)}
        self._flags = torch.zeros(len(self.params), dtype=torch.float32, device=self.params[0].device)
        self._flags_host = None
        self._flags_copied = None  # event behind the last asynchronous copy out of the pinned flag buffer
        self._pending, self._next, self._handles, self._fired = [], 0, [], set()
        self._events = [[] for _ in self.buckets]
        self._hold, self._held = False, []
        self._cuda = self.params[0].is_cuda
        self._comm = torch.cuda.Stream(device=self.params[0].device) if (self._cuda and self.ws > 1) else None
        self.n_collectives = 0
        self._timing = []  # (bucket, start event, end event) of the last step's bucket all-reduces, on the communication stream
        self.payload_bytes = sum(f.numel() * 4 for f in self.flat)  # what one step's bucket all-reduces carry (+ 4 B per parameter of flags)
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in self.params] if hooks else []

    def close(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []

    def begin_step(self):
        self._pending = [len(ps) for ps in self.buckets]
        self._next = 0
        self._handles, self._fired, self.n_collectives = [], set(), 0
        self._events = [[] for _ in self.buckets]
        self._hold, self._held = False, []
        self._timing = []
        for flat in self.flat:
            flat.zero_()
        for p in self.params:
            p.grad = self.views[p]
        if self._cuda and self.train_ctx is not None:  # kernels that scatter a gradient straight into its bucket view ask for it here
            self.train_ctx.sink = self                  # (field_ops.scatter_to_sink, through the step's TrainContext)

    def view_for(self, p):
        return self.views.get(p)

    def _on_grad(self, p):
        if p.grad is not None and p.grad.data_ptr() != self.views[p].data_ptr():  # autograd replaced the view: fold it back in
            self.views[p].copy_(p.grad)
            p.grad = self.views[p]
        self.mark_ready(p)

    def hold(self, on):
        """A step made of several backward passes (train_step.RenderTrainStep: LiDAR pass, then camera pass): while `on`, a
        gradient that arrives is only noted -- a parameter both passes reach is final after the last one.  `release_held()` after
        the last pass marks what the later passes did not touch."""
        self._hold = bool(on)

    def release_held(self):
        held, self._held, self._hold = self._held, [], False
        if held and self._cuda:
            from nvsf import field_ops
            field_ops.sync_side_streams()  # held scatters ran on the side stream; the events below are recorded on this one
        for p in held:
            self.mark_ready(p)

    def mark_ready(self, p):
        """The gradient of `p` (in its bucket view) is final.  Called by the hook, or by a kernel wrapper that scattered straight
        into the view (field_ops.scatter_to_sink, behind a table's last scatter of the pass -- on the side stream with
        TrainContext.overlap: the collective then waits for that stream)."""
        if self._hold:
            self._held.append(p)
            return
        if p in self._fired:
            return
        self._fired.add(p)
        b = self.bucket_of[p]
        if self._comm is not None:  # gradients are produced on the main stream or on the table-scatter side stream: the
            ev = torch.cuda.Event()  # collective (issued on its own stream) waits for exactly the producers of its bucket
            ev.record()
            self._events[b].append(ev)
        self._pending[b] -= 1
        self._launch_ready()

    def _launch_ready(self, force=False):
        """Collectives are matched across ranks by their sequence, so buckets are issued strictly in bucket order: bucket b goes
        out once it is complete AND every bucket before it has gone out (a rank on which some parameter never receives a
        gradient issues the rest in `finish`, in the same order)."""
        while self._next < len(self.buckets) and (force or self._pending[self._next] == 0):
            b = self._next
            self._next += 1
            if self.ws > 1:
                if self._comm is not None:
                    if force:  # a bucket closed by `finish`: everything queued on the calling stream so far belongs to it
                        self._comm.wait_stream(torch.cuda.current_stream())
                    for ev in self._events[b]:
                        self._comm.wait_event(ev)
                    with torch.cuda.stream(self._comm):
                        # RCCL runs the collective on a stream of its own; work.wait() makes THIS (communication) stream wait for
                        # it without blocking the host, so the event pair brackets the collective's device time
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        work = dist.all_reduce(self.flat[b], op=dist.ReduceOp.SUM, async_op=True)
                        work.wait()
                        t1.record()
                        self._handles.append(work)
                        self._timing.append((b, t0, t1))
                else:
                    self._handles.append(dist.all_reduce(self.flat[b], op=dist.ReduceOp.SUM, async_op=True))
                self.n_collectives += 1

    def allreduce_ms(self):
        """Device time of each bucket all-reduce of the LAST step on the communication stream, [(bucket, MB, ms)] -- waits for them.
        (RCCL on a GPU node; empty on the CPU / gloo path.)  For the scaling record: the ring estimate is
        2 (W - 1) / W x payload / per-link rate."""
        out = []
        for b, t0, t1 in self._timing:
            t1.synchronize()
            out.append((b, self.flat[b].numel() * 4 / 1e6, t0.elapsed_time(t1)))
        return out

    def finish(self):
        if self._cuda:
            from nvsf import field_ops
            if self.train_ctx is not None:
                self.train_ctx.sink = None
            field_ops.sync_side_streams()
        self._launch_ready(force=True)
        # "somebody produced a gradient" flags: written on the host (pinned) and copied without blocking
        #  the copy is asynchronous and, when every parameter fired, nothing below waits for it: the pinned buffer may be
        # rewritten only after the PREVIOUS step's copy has left it -- an event behind the copy, waited for (on the host, normally long
        # past) before the buffer is touched again
        if self._flags_host is None:
            self._flags_host = torch.zeros(len(self.params), dtype=torch.float32)
            if self._cuda:
                self._flags_host = self._flags_host.pin_memory()
            self._flags_copied = None
        if self._flags_copied is not None:
            self._flags_copied.synchronize()
        self._flags_host.zero_()
        for p in self._fired:
            self._flags_host[self._index[p]] = 1.0
        self._flags.copy_(self._flags_host, non_blocking=True)
        if self._cuda:
            self._flags_copied = torch.cuda.Event()
            self._flags_copied.record()
        if self.ws > 1:
            self._handles.append(dist.all_reduce(self._flags, op=dist.ReduceOp.MAX, async_op=True))
            self.n_collectives += 1
            for h in self._handles:
                h.wait()
            for flat in self.flat:
                flat.div_(self.ws)
        # A parameter is touched if ANY rank produced a gradient for it.  Every parameter this rank fired is touched, whatever the
        # others did: only when some parameter did NOT fire here does the answer depend on the reduced flags -- and only then are they
        # read back (one device->host sync; a step that uses every parameter on every rank, the usual case, has none).  The MAX
        # all-reduce above is issued regardless: collectives are matched across ranks by sequence, and another rank may need it.
        local = [1.0 if p in self._fired else 0.0 for p in self.params]
        touched = self._flags.tolist() if (self.ws > 1 and not all(local)) else local
        for p, t in zip(self.params, touched):
            if t == 0.0:
                p.grad = None
        return self.n_collectives
