"""CPU tests of the host function that picks the step order of the mirrored causal forward
(attention_fwd_v2.hip fwd_own_first_tiles, exported as mfa_forward_order_tiles): the routed
threshold, the development override, the kernels that never take the second order, and that
the plan does not change with it.  The GPU twin is test_forward_order_gpu.py."""
import os
import subprocess
import sys

import mfa_amd as mfa

# The routed threshold (light-block key tiles; DESIGN.md §3, "Own tiles first").
ROUTED_TILES = 10

order = mfa.lib.mfa_forward_order_tiles


def test_routed_threshold(monkeypatch):
    monkeypatch.delenv("MFA_FWD_ORDER", raising=False)
    assert order(1, 0, 0) == ROUTED_TILES


def test_override_sets_the_threshold(monkeypatch):
    monkeypatch.setenv("MFA_FWD_ORDER", "0")
    assert order(1, 0, 0) == 0
    monkeypatch.setenv("MFA_FWD_ORDER", "6")
    assert order(1, 0, 0) == 6
    monkeypatch.setenv("MFA_FWD_ORDER", "64")
    assert order(1, 0, 0) == 64
    monkeypatch.setenv("MFA_FWD_ORDER", "-3")
    assert order(1, 0, 0) == 0


def test_other_kernels_keep_the_shared_first_order(monkeypatch):
    # Adjacent pairs, INT8 / INT4 K/V widened on load and sparse ranges, whatever the switch says.
    for env in (None, "6"):
        if env is None:
            monkeypatch.delenv("MFA_FWD_ORDER", raising=False)
        else:
            monkeypatch.setenv("MFA_FWD_ORDER", env)
        assert order(0, 0, 0) == 0
        assert order(1, 1, 0) == 0
        assert order(1, 2, 0) == 0
        assert order(1, 0, 1) == 0
        assert order(0, 0, 1) == 0


def test_plan_does_not_depend_on_the_order(monkeypatch):
    # B1 H16 S4096 D128 causal: one launch of the mirrored kernel, both orders inside it.
    base = mfa.AttentionDescriptor.make(low_precision=True, precision=mfa.Precision.FP16,
                                        causal=True)
    d = mfa.MultiHeadDescriptor.make(base, 1, 16, 4096, 128)
    plans = []
    for env in ("0", "4", "64"):
        monkeypatch.setenv("MFA_FWD_ORDER", env)
        plans.append(mfa.multihead_plan(d))
    monkeypatch.delenv("MFA_FWD_ORDER")
    plans.append(mfa.multihead_plan(d))
    assert [r["name"] for r in plans[0]] == \
        ["mfa_fwd2_share_kernel<F16, 128, 64, true, true, true, true>"]
    assert all(p == plans[0] for p in plans)


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "metal-flash-attention-plus_amd", "python"))
import mfa_amd as mfa
print(mfa.lib.mfa_forward_order_tiles(1, 0, 0))
"""


def test_override_is_a_development_switch():
    # Without MFA_DEV=1 the process environment cannot change the order (mfa_launch.h dev_env).
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MFA_")}
    env["MFA_FWD_ORDER"] = "37"
    r = subprocess.run([sys.executable, "-c", _CHILD, repo], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.strip().splitlines()[-1]) == ROUTED_TILES
