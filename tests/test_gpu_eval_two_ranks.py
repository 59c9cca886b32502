"""GPU (-m gpu): validation sharded over two ranks (both on cuda:0, gloo transport so it runs on a 1-GPU box): three frames split 2 + 1 by
make_val_loaders, summed and counted across the ranks by ModelWrapper.validation_epoch_end, must give the single-rank result.  The ranks
add the same three float32 terms in another order, so every value has to agree within 4 ulp of float32.  Each rank is a child process of
its own (this file run as a script) under its own ``timeout``."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODEL = {"loss": {"supervised_method": "sparse-silog", "supervised_num_scales": 1, "supervised_loss_weight": 1.0,
                  "edges_depth_edge_loss_all_scales": True}, "params": {"crop": "garg"}}


def _config(folder):
    from mindtheedge_amd.utils.config import load_config
    return load_config(None, {"model": MODEL, "datasets": {"validation": {"dataset": ["KITTI"], "path": [folder], "depth_type": ["groundtruth"],
                                                                           "split": [os.path.join(folder, "val_files.txt")]}}})


def _validate(folder, rank, world):
    import torch
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.datasets.kitti_edges import make_val_loaders
    from mindtheedge_amd.models.model_wrapper import ModelWrapper
    from mindtheedge_amd.trainers.trainer import Trainer
    K.set_compute_dtype("bf16")
    torch.cuda.set_device(0)
    cfg = _config(folder)
    wrap = ModelWrapper(cfg).cuda()                      # config.arch.seed: every process builds the same weights
    loaders = make_val_loaders(cfg, rank, world)
    (res,) = Trainer(max_epochs=1).validate(loaders, wrap)
    return res, [len(l.indices()) for l in loaders]


def _child(rank, port, folder, out):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        res, counts = _validate(folder, rank, 2)
        with open(out, "w") as f:
            json.dump({"metrics": res, "frames": counts}, f)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.gpu
def test_two_ranks_give_the_single_rank_validation(tmp_path):
    sys.path.insert(0, HERE)
    import eval_prep_ref as R
    folder = os.path.join(str(tmp_path), "KITTI_tiny")
    R.write_split(folder, n=3)
    single, counts = _validate(folder, 0, 1)
    assert counts == [3] and len(single) == 28 + 9
    port = _free_port()
    outs = [os.path.join(str(tmp_path), "rank%d.json" % r) for r in range(2)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), str(r), str(port), folder, outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], logs
    got = [json.load(open(o)) for o in outs]
    assert [g["frames"] for g in got] == [[2], [1]]
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))
    assert sorted(got[0]["metrics"]) == sorted(got[1]["metrics"])
    assert all(same(v, got[1]["metrics"][k]) for k, v in got[0]["metrics"].items())       # both ranks hold the reduced result
    assert sorted(got[0]["metrics"]) == sorted(single)
    for k, v in single.items():
        w = got[0]["metrics"][k]
        ulp = float(np.spacing(np.float32(max(abs(v), abs(w)))))
        print(k, v, w, abs(v - w) / ulp if ulp else 0.0)
        assert (np.isnan(v) and np.isnan(w)) or abs(v - w) <= 4 * ulp, (k, v, w)


if __name__ == "__main__":
    _child(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4])
