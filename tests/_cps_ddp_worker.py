"""Worker of tests/test_gpu_cps.py::test_two_ranks_train_both_networks_as_one_process_on_the_mean_gradient.

    python tests/_cps_ddp_worker.py rank <out.pt> <save_dir>         one rank of a 2-process cps job built by ``semi_seg/main.py``'s
                                                                     ``build_trainer`` (RANK / WORLD_SIZE / MISEG_DDP_BACKEND=gloo
                                                                     from the environment, both ranks on cuda:0), one epoch of 2 steps
    python tests/_cps_ddp_worker.py reference <out.pt> <save_dir>    ONE process that builds both ranks' trainers (same initial
                                                                     weights, each rank's data) and, step by step, computes rank 1's
                                                                     gradient, then rank 0's, and lets rank 0's optimiser step on
                                                                     (g0 + g1) / 2 -- what the all-reduce (a sum) and the reducer's
                                                                     division leave in the flat gradient of either rank

Both save the flat parameter buffer before and after (it spans network A and network B), each network's span in it and network A's
BatchNorm buffers.
"""
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")
sys.path[:0] = [ROOT, PKG]
os.environ.setdefault("MISEG_PROGRESS", "0")

import torch  # noqa: E402

STEPS = 2


def arguments(save):
    return ["Trainer.name=cps", f"Trainer.save_dir={save}", "Trainer.device=cuda", "Trainer.max_epoch=1", f"Trainer.num_batches={STEPS}",
            "Data.size=64", "Data.name=synthetic", "LabeledData.batch_size=2", "UnlabeledData.batch_size=3", "Optim.lr=0.001"]


def spans(tr):
    """{network: (first, one past the last) float of its parameters in the flat buffer}: the optimiser was handed A's, then B's."""
    flat = tr._optimizer.flat
    flat.ensure()
    out = {}
    for net, model in (("a", tr._model), ("b", tr._model_b)):
        where = [(flat.offset_of(p), p.numel()) for p in model.parameters()]
        out[net] = (min(o for o, _ in where), max(o + n for o, n in where))
    assert out["a"][1] <= out["b"][0], out
    return out


def result(tr, init, steps):
    torch.cuda.synchronize()
    return {"steps": steps, "init": init, "param": tr._optimizer.flat.flat_param.detach().cpu().clone(), "span": spans(tr),
            "bn_a": torch.cat([b.detach().float().reshape(-1).cpu() for b in tr._model.buffers()])}


def rank(out, save):
    from semi_seg.main import build_trainer
    tr = build_trainer(arguments(save))
    try:
        assert tr._grad_reducer is not None and tr._grad_reducer.flat is tr._optimizer.flat
        span = spans(tr)
        assert span["b"][1] <= tr._optimizer.flat.total and sum(end - start for _, _, start, end in tr._grad_reducer.buckets) == tr._optimizer.flat.total      # the buckets cover both networks
        init = tr._optimizer.flat.flat_param.detach().cpu().clone()
        tr._run_epoch()
        torch.save(result(tr, init, STEPS), out)
        torch.distributed.barrier()
    finally:
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        shutil.rmtree(os.path.join(PKG, "semi_seg", "runs", save), ignore_errors=True)


class _LocalGradient:
    """Stands where a ``GradReducer`` stands in rank 1's epocher: the pass only leaves its gradient."""

    def __init__(self, flat):
        self.flat, self.grad = flat, None

    def prepare(self):
        self.flat.ensure()

    def finish(self):
        self.flat.collect()
        self.grad = self.flat.flat_grad.detach().clone()


class _MeanWith(_LocalGradient):
    """... and in rank 0's: its gradient plus ``other``'s, halved."""

    def __init__(self, flat, other):
        super().__init__(flat)
        self.other = other

    def finish(self):
        self.flat.collect()
        self.flat.flat_grad.add_(self.other.grad).div_(2)


def reference(out, save):
    import bench
    from miseg_amd import packcache
    from semi_seg.main import build_trainer
    trainers = []
    try:
        for r in range(2):
            os.environ["RANK"] = str(r)                  # no WORLD_SIZE: no process group, the rank only picks the data
            trainers.append(build_trainer(arguments(f"{save}_{r}")))
            trainers[-1].to(trainers[-1]._device)        # what ddp.attach does for a rank, and start_training for a single process
        t0, t1 = trainers
        o0, o1 = t0._optimizer, t1._optimizer
        o0.flat.ensure()
        o1.flat.ensure()
        init = o0.flat.flat_param.detach().cpu().clone()
        assert torch.equal(init, o1.flat.flat_param.detach().cpu())
        e0, e1 = t0._make_epocher(), t1._make_epocher()
        e1._reducer = _LocalGradient(o1.flat)
        e0._reducer = _MeanWith(o0.flat, e1._reducer)
        e0._TAPE_DEFAULT = e1._TAPE_DEFAULT = False
        t0._model_b.train()
        t1._model_b.train()
        d0, d1 = bench.StepDriver(e0), bench.StepDriver(e1)
        for _ in range(STEPS):
            d1.step()
            d0.step()
            torch.cuda.synchronize()
            with torch.no_grad():                        # rank 1 took a step of its own on g1 alone: give it rank 0's state instead
                o1.flat.flat_param.copy_(o0.flat.flat_param)
                for mine, theirs in zip(o1._m + o1._v, o0._m + o0._v):
                    mine.copy_(theirs)
            packcache.PACK_CACHE.invalidate()
        d0.close()
        d1.close()
        torch.save(result(t0, init, STEPS), out)
    finally:
        for r in range(2):
            shutil.rmtree(os.path.join(PKG, "semi_seg", "runs", f"{save}_{r}"), ignore_errors=True)


if __name__ == "__main__":
    {"rank": rank, "reference": reference}[sys.argv[1]](sys.argv[2], sys.argv[3])
