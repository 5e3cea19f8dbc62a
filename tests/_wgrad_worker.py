"""Child process of test_hip_wgrad.py:  python tests/_wgrad_worker.py <cases.pt> <out.pt>

Loads the cases the parent prepared on the CPU (tests/_wgrad_cases.py), runs each on the device once, in order, and saves the gradients
(moved to the CPU) by case name.  The switches ODEHIP_WGRAD_WINO / ODEHIP_WGRAD_WINO5 are read once per process by the library, which is
why this is a process of its own; the parent chooses the environment and this file sets none.  The first error ends the process with a
non-zero status: nothing further is launched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(cases_path, out_path):
    import torch
    import _wgrad_cases as wc
    cases = torch.load(cases_path)
    dev = torch.device("cuda:0")
    out = {}
    for name, spec in cases.items():
        out[name] = wc.run_on_device(dev, spec)
        torch.cuda.synchronize()
        print(f"{name}: done", flush=True)
    torch.save(out, out_path)


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
