"""Child process of tests/test_gpu_envelope_entries.py: IRON_H2_OVERFLOW=error (read once per process, csrc/envelope.hip).
overflow -> the next call on the handle is IRON_ERR_RANGE, and so is the one after it -> force_exact(True) -> the next call succeeds
on the exact core and is right -> force_exact(False) clears the status and the handle is back on the default core."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
assert os.environ.get("IRON_H2_OVERFLOW") == "error"

import torch  # noqa: E402

torch.set_grad_enabled(False)
from iron_amd import _lib  # noqa: E402
import _envelope_cases as E  # noqa: E402

dev = torch.device("cuda", 0)
case = E.get_case("sdf/a")
idx = E.arrangements(case)["n300"]
x = case.inputs[0][idx].contiguous().to(dev)
net = copy.deepcopy(case.net).to(dev)
clean_status = {"overflow_seen": False, "exact_core": False, "pending": False}
assert net.numeric_status() == clean_status
first = net.sdf(x)
assert net.numeric_status()["pending"] and not bool(torch.isfinite(first).all())
for attempt in range(2):        # the handle refuses work, and keeps refusing
    try:
        net.sdf(x)
    except _lib.IronError as e:
        assert "fp16 range" in str(e), str(e)
    else:
        raise AssertionError("call %d after the overflow did not return IRON_ERR_RANGE" % (attempt + 1))
st = net.numeric_status()
assert st["overflow_seen"] and st["pending"] and not st["exact_core"], st
net.force_exact(True)           # the remedy iron_strerror names
st = net.numeric_status()
assert st["overflow_seen"] and st["exact_core"] and not st["pending"], st
s, f, g = net.get_all(x, is_training=False)
problems, any_bad, worst, _ = E.judge(case, idx, {"sdf": s, "feature": f, "gradient": g}, exact=True)
assert not problems and not any_bad, problems
assert net.numeric_status()["exact_core"]
net.force_exact(False)
assert net.numeric_status() == clean_status, net.numeric_status()
clean = E.arrangements(case)["n1"]
one = net.sdf(case.inputs[0][clean].contiguous().to(dev))      # a clean row on the default core again: right, and no flag
problems, any_bad, _, _ = E.judge(case, clean, {"sdf": one})
assert not problems and not any_bad and net.numeric_status() == clean_status
# a second handle of the process is not affected by the first one's state, and an in-range call never errors in this mode
other = copy.deepcopy(E.get_case("sdf/h").net).to(dev)
idx_h = E.arrangements(E.get_case("sdf/h"))["n300"]
for _ in range(2):
    out = other.sdf(E.get_case("sdf/h").inputs[0][idx_h].contiguous().to(dev))
assert other.numeric_status() == clean_status and bool(torch.isfinite(out).all())
print("ENVELOPE_ERROR_CHECK OK worst ratio on the exact core after force_exact: %.2f" % max(worst.values()))
