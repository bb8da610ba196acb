"""From rocprofv3 kernel traces (run_kernel_trace.csv of `--kernel-trace --stats` runs of bench.py):
per training iteration, the count and summed duration of every kernel other than the train, rollout
step, gradient-reduce and fused-Adam kernels, and the GPU idle time between the iteration's last
env step (k_sample_env_r) and its first k_mlp_train_x3 launch.  Averages over the last 20
iterations (the bench's timed ones).  usage: python tools/trace_glue.py TRACE.csv [TRACE.csv ...]"""
import collections
import csv
import sys

MAIN = ("k_mlp_train_x3", "k_sample_env_r", "k_policy_mfma", "k_grad_reduce_blocks", "multi_tensor_apply")


def iterations(path):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                  for r in csv.DictReader(open(path)))
    its, cur = [], []
    for row in rows:  # an iteration ends where a rollout kernel follows the update's kernels
        rollout = "k_sample_env_r" in row[2] or "k_policy_mfma" in row[2]
        if rollout and any("k_mlp_train" in x[2] for x in cur):
            its.append(cur)
            cur = []
        cur.append(row)
    its.append(cur)
    return [it for it in its if any("k_mlp_train" in x[2] for x in it) and any("k_sample_env_r" in x[2] for x in it)]


def main():
    for path in sys.argv[1:]:
        its = iterations(path)[-20:]
        n = len(its)
        count = dur = span = idle = 0
        names = collections.Counter()
        for it in its:
            others = [x for x in it if not any(m in x[2] for m in MAIN)]
            count += len(others)
            dur += sum(e - s for s, e, _ in others)
            for s, e, name in others:
                names[name[:80]] += e - s
            t0 = max(e for s, e, name in it if "k_sample_env_r" in name)
            t1 = min(s for s, e, name in it if "k_mlp_train_x3" in name and s > t0)
            busy = sum(min(e, t1) - max(s, t0) for s, e, _ in it if e > t0 and s < t1)
            span += t1 - t0
            idle += t1 - t0 - busy
        print(path)
        print(f"  {n} iterations: {count / n:.1f} other kernels per iteration, {dur / n / 1e3:.1f} us")
        print(f"  last env step -> first train launch: {span / n / 1e3:.1f} us, of which idle {idle / n / 1e3:.1f} us")
        for name, v in names.most_common(12):
            print(f"    {v / n / 1e3:8.1f} us  {name}")


if __name__ == "__main__":
    main()
