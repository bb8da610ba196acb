"""Two PPO iterations with the KL early stop on 64 coop envs; saves every net's flat parameters
(<out>.npy) and the kl_stops record (<out>.json) (tests/test_target_kl_gpu.py).  tau comes from a first
run with target_kl=inf: three quarters of the largest head's mean KL after four actor steps, over 1.5, so
that head stops by its fourth step.
--nccl-world1: one rank on RCCL with the data-parallel collectives forced on (as tests/dp_worker.py): the
KL sums then travel through the update's all-reduces; a one-rank SUM is the identity."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--nccl-world1", action="store_true")
a = ap.parse_args()
torch.cuda.set_device(0)
if a.nccl_world1:
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29800 + os.getpid() % 90))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from mhppo import ppo  # noqa: E402
    ppo.set_force_collectives(True)
from mhppo.algo import Algo_PPO  # noqa: E402
from mhppo.env import VecCrosswalk  # noqa: E402
from mhppo.models import Model_PPO  # noqa: E402


def run(n, tau):
    venv = VecCrosswalk("coop", 64, 2, 1, 2, seed_base=11, device="cuda:0")
    torch.manual_seed(0)
    algo = Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, seed=3, target_kl=tau)
    algo.train(n)
    algo.curves()
    return algo


first = run(1, float("inf")).kl_stops[0]
tau = 0.75 * max(v["approx_kl"][3] for k, v in first.items() if k != "iteration") / 1.5
algo = run(2, tau)
np.save(a.out + ".npy", np.concatenate([net.flat().cpu().numpy() for net in algo.nets()]))
with open(a.out + ".json", "w") as f:
    json.dump({"tau": tau, "kl_stops": algo.kl_stops}, f)
if dist.is_initialized():
    dist.barrier()
    dist.destroy_process_group()
