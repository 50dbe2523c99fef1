"""CPU checks of the device-side evaluation's public surface (no GPU): the C ABI entry and its struct, the C++
header's evaluate / metrics in standalone mode, the count limbs of the all-reduce as a stand-alone program (also
under the address and undefined-behaviour sanitizers), the EarlyStopper rule, and the new UnifiedConfig fields."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "lbfgs-ffnn_amd", "csrc")

TU = r"""
#include "lbfgs_amd/hip_backend.hpp"

static_assert(sizeof(lbf_eval_result) == 40, "lbf_eval_result layout");

int main() {
  UnifiedLauncher<HipBackend> launcher;
  launcher.addLayer<784, 128, hip_mlp::ReLU>();
  launcher.addLayer<128, 10, hip_mlp::Linear>();
  launcher.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
  launcher.buildNetwork();
  hip_mlp::HipNetwork &net = launcher.getWrapper().getInternal();
  std::vector<long long> conf;
  hip_mlp::EvalResult a = net.evaluate(nullptr, nullptr, 0);
  hip_mlp::EvalResult b = net.evaluate(nullptr, nullptr, 0, 3, &conf, nullptr);
  hip_mlp::EvalResult c = launcher.metrics(true);
  hip_mlp::EvalResult d = launcher.metrics(false, 2, &conf);
  return int(a.rows + b.topk + c.correct) + (d.accuracy() + d.topk_accuracy() + d.loss > 0.0 ? 1 : 0) + d.k;
}
"""

LIMBS = r"""
#include "eval_limbs.hpp"

#include <cstdio>

int main() {
  using namespace lbf;
  const unsigned long long vals[] = {0ull, 1ull, (1ull << 16) - 1, 1ull << 16, (1ull << 24) + 1, (1ull << 47) + 12345ull};
  int bad = 0;
  for (unsigned long long v : vals) {
    float w[kEvalLimbs];
    eval_limbs_split(v, w);
    for (int i = 0; i < kEvalLimbs; ++i) bad += !(w[i] >= 0.0f && w[i] < 65536.0f);
    if ((unsigned long long)eval_limbs_merge(w) != v) {
      std::printf("round trip of %llu gives %lld\n", v, eval_limbs_merge(w));
      ++bad;
    }
  }
  // 256 ranks: the limbs summed in fp32 (any order: every partial sum is an integer below 2^24) give the exact
  // integer sum, for the listed values and for the largest limbs a rank can send
  for (int pass = 0; pass < 2; ++pass) {
    float sum[kEvalLimbs] = {0.0f, 0.0f, 0.0f};
    unsigned long long want = 0;
    for (int r = 0; r < kEvalMaxRanks; ++r) {
      const unsigned long long v = pass == 0 ? vals[r % 6] + (unsigned long long)r * 977ull : (1ull << 48) - 1 - (unsigned long long)r;
      float w[kEvalLimbs];
      eval_limbs_split(v, w);
      for (int i = 0; i < kEvalLimbs; ++i) sum[i] += w[i];
      want += v;
    }
    for (int i = 0; i < kEvalLimbs; ++i) bad += !(sum[i] < 16777216.0f);
    if ((unsigned long long)eval_limbs_merge(sum) != want) {
      std::printf("pass %d: sum over ranks gives %lld, want %llu\n", pass, eval_limbs_merge(sum), want);
      ++bad;
    }
  }
  std::printf("limbs %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
"""


def test_cpp_evaluate_and_metrics_compile_standalone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{INCLUDE}", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_count_limbs_round_trip_and_rank_sum(tmp_path, san):
    src, exe = tmp_path / "limbs.cpp", tmp_path / "limbs"
    src.write_text(LIMBS)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, f"-I{CSRC}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "limbs ok" in r.stdout, r.stdout + r.stderr


def test_library_exports_evaluate(pkg):
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (lbf_\w+)", out))
    assert "lbf_mlp_evaluate" in exported and hasattr(L, "lbf_mlp_evaluate")
    assert "lbf_mlp_evaluate" in pkg._lib.EXPORTS
    hdr = open(os.path.join(INCLUDE, "lbfgs_amd.h")).read()
    assert re.search(r"\bint\s+lbf_mlp_evaluate\s*\(", hdr) and re.search(r"typedef\s+struct\s+lbf_eval_result\b", hdr)
    assert "unified_launcher.hpp:154-199" in hdr   # the reference lines the entry replaces
    assert re.search(r"#define\s+LBF_ABI_VERSION\s+3\b", hdr) and L.lbf_abi_version() == 3
    # null handles are reported, not dereferenced
    res = pkg._lib.EvalResultC()
    import ctypes as C
    assert L.lbf_mlp_evaluate(None, None, None, None, None, 0, 1.0, 1, 0, None, None, None, None) == 1
    assert L.lbf_mlp_evaluate(None, None, None, None, None, 4, 1.0, 1, 0, C.byref(res), None, None, None) == 1
    assert C.sizeof(pkg._lib.EvalResultC) == 40


def _run(stopper, seq):
    """Feed (loss, accuracy) pairs; return the index of the evaluation at which it asks to stop (None: never)."""
    for i, (loss, acc) in enumerate(seq):
        if stopper.update(i, loss, acc):
            return i
    return None


def test_early_stopper_rule(pkg):
    ES = pkg.EarlyStopper
    # improving forever: never stops, the best is the last
    s = ES(patience=2)
    assert _run(s, [(1.0 / (i + 1), 0.0) for i in range(50)]) is None and s.best_iteration == 49
    # a plateau of exactly `patience` evaluations stops at its last one; one shorter does not
    s = ES(patience=3)
    assert _run(s, [(5.0, 0), (4.0, 0), (4.5, 0), (4.2, 0), (4.1, 0), (1.0, 0)]) == 4
    assert s.best_iteration == 1 and s.best_loss == 4.0
    s = ES(patience=3)
    assert _run(s, [(5.0, 0), (4.0, 0), (4.5, 0), (4.2, 0), (3.9, 0), (3.95, 0), (3.99, 0)]) is None
    assert s.best_iteration == 4 and s.stale == 2
    # ties are not improvements, and the earliest of equal values stays the best
    s = ES(patience=2)
    assert _run(s, [(3.0, 0), (3.0, 0), (3.0, 0), (1.0, 0)]) == 2 and s.best_iteration == 0
    # a NaN is not an improvement
    s = ES(patience=1)
    assert _run(s, [(3.0, 0), (float("nan"), 0)]) == 1 and s.best_iteration == 0
    # monitor="accuracy": higher is better, the loss is ignored
    s = ES(patience=2, monitor="accuracy")
    assert _run(s, [(9.0, 0.1), (8.0, 0.3), (1.0, 0.3), (0.5, 0.2), (0.1, 0.9)]) == 3
    assert s.best_iteration == 1 and s.best_accuracy == 0.3
    s = ES(patience=2, monitor="accuracy")
    assert _run(s, [(1.0, 0.1), (2.0, 0.2), (3.0, 0.3), (4.0, 0.4)]) is None and s.best_iteration == 3
    # patience=0 never stops, and still tracks the best
    s = ES(patience=0)
    assert _run(s, [(1.0, 0), (2.0, 0), (3.0, 0), (0.5, 0), (4.0, 0)]) is None and s.best_iteration == 3
    with pytest.raises(pkg.LbfError):
        ES(patience=1, monitor="f1")
    with pytest.raises(pkg.LbfError):
        ES(patience=-1)


def test_config_defaults_and_gd_rejects_monitoring_before_the_device(pkg):
    c = pkg.UnifiedConfig()
    assert c.eval_every == 0 and c.patience == 0 and c.monitor == "loss" and c.restore_best is True
    # net = data = None: an optimize() that went on to the device would fail on them with another error
    for opt in (pkg.UnifiedGD(), pkg.UnifiedSGD()):
        with pytest.raises(pkg.LbfError, match="eval_every"):
            opt.optimize(None, None, pkg.UnifiedConfig(eval_every=1))
    # a missing test split is an LbfError too, raised before any device work
    for opt in (pkg.UnifiedLBFGS(), pkg.UnifiedSLBFGS()):
        with pytest.raises(pkg.LbfError, match="test split"):
            opt.optimize(None, None, pkg.UnifiedConfig(eval_every=1))
    assert callable(pkg.Mlp.evaluate) and callable(pkg.UnifiedLauncher.metrics)
    assert [f for f in pkg.EvalResult.__dataclass_fields__][:6] == ["loss", "rows", "correct", "topk", "k", "accuracy"]
