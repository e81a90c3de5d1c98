"""CPU: the gradient-sink contract of the table nodes (field_ops.announce at forward, field_ops.scatter_to_sink at backward,
TrainContext.end_pass after a backward pass), driven through a toy autograd.Function and a recording sink -- no kernel involved."""
import torch

from nvsf import field_ops as ops


class RecordingSink:
    """A sink on the calling stream (TrainContext.overlap off): `.grad` buffers, and the order of scatters and mark_ready calls."""

    def __init__(self):
        self.log = []  # ("scatter" | "ready", id(table))

    def view_for(self, p):
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def mark_ready(self, p):
        self.log.append(("ready", id(p)))


class ScaleFn(torch.autograd.Function):
    """y = x * sum(tables): dL/dtable = g * x for every table, scattered into the sink when the step has one."""

    @staticmethod
    def forward(ctx, x, train_ctx, *tables):
        ops.announce(ctx, train_ctx, tables)
        ctx.save_for_backward(x)
        ctx.n_tables = len(tables)
        return x * sum(t.detach() for t in tables)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gt = g * x

        def scatter(views, pool):
            for view, p in zip(views, ctx.tables):
                view.add_(gt)
                ctx.train_ctx.sink.log.append(("scatter", id(p)))
        if ops.scatter_to_sink(ctx, (x, gt), scatter):
            return (None, None) + (None,) * ctx.n_tables
        return (None, None) + (gt,) * ctx.n_tables


def _step(sink=None):
    """A TrainContext inside a counted step, attached to a module as RenderTrainStep does."""
    tctx = ops.TrainContext()
    tctx.sink = sink
    tctx.begin_step()
    mod = torch.nn.Module()
    mod.__dict__["_train_ctx"] = tctx
    return tctx, mod


def _table():
    return torch.nn.Parameter(torch.randn(4))


def test_forward_with_grad_announces():
    tctx, mod = _step()
    p = _table()
    ScaleFn.apply(torch.randn(4), ops.train_context(mod), p)
    assert len(tctx.left) == 1 and tctx.left[p] == 1


def test_forward_without_grad_announces_nothing():
    tctx, mod = _step()
    p = _table()
    with torch.no_grad():
        assert ops.train_context(mod) is None
        ScaleFn.apply(torch.randn(4), ops.train_context(mod), p)
    assert tctx.left == {}


def test_one_mark_ready_per_table_behind_its_last_scatter():
    sink = RecordingSink()
    tctx, mod = _step(sink)
    p = _table()
    x1, x2 = torch.randn(4), torch.randn(4)
    y = ScaleFn.apply(x1, ops.train_context(mod), p) + ScaleFn.apply(x2, ops.train_context(mod), p)
    assert tctx.left[p] == 2
    y.sum().backward()
    assert sink.log == [("scatter", id(p)), ("scatter", id(p)), ("ready", id(p))]
    assert torch.equal(p.grad, x1 + x2)
    assert tctx.end_pass() == set() and sink.log[-1] == ("ready", id(p)) and len(sink.log) == 3


def test_frozen_table_gets_no_grad_and_no_scatter():
    sink = RecordingSink()
    tctx, mod = _step(sink)
    p, q = _table(), _table()
    q.requires_grad_(False)
    x = torch.randn(4)
    ScaleFn.apply(x, ops.train_context(mod), p, q).sum().backward()
    assert q.grad is None and all(i != id(q) for _, i in sink.log)
    assert sink.log == [("scatter", id(p)), ("ready", id(p))] and torch.equal(p.grad, x)
    assert list(tctx.left) == [p]


def test_without_a_sink_the_gradient_goes_through_autograd():
    tctx, mod = _step()
    p = _table()
    x1, x2 = torch.randn(4), torch.randn(4)
    (ScaleFn.apply(x1, ops.train_context(mod), p) + ScaleFn.apply(x2, ops.train_context(mod), p)).sum().backward()
    assert torch.allclose(p.grad, x1 + x2)
    assert sum(tctx.left.values()) == 0 and tctx.end_pass() == set()


def test_end_pass_marks_a_table_whose_last_scatter_never_came():
    sink = RecordingSink()
    tctx, mod = _step(sink)
    p, r = _table(), _table()
    used = ScaleFn.apply(torch.randn(4), ops.train_context(mod), p)
    ScaleFn.apply(torch.randn(4), ops.train_context(mod), p, r)  # announced, never reached by backward
    used.sum().backward()
    assert sink.log == [("scatter", id(p))]  # not final yet: one scatter is still expected
    assert tctx.end_pass() == {p, r} and tctx.leftover == {p, r}
    assert sink.log == [("scatter", id(p)), ("ready", id(p))]  # r received nothing: nothing to wait for
    assert tctx.left == {}
