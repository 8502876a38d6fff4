"""The default forward instantiation in the built library, read with tools/kernel_census.py: no scratch, at most 256 VGPRs,
and no more SGPR-to-VGPR-lane moves (v_readlane_b32 / v_writelane_b32) inside its key-tile loop than the count the
production kernel shipped with (profiles/fwd_production.md), so that a later change cannot bring the spills back unnoticed.
The in-stream LDS-DMA of that kernel pads only the one wait state M0 needs (dma16_issue_s), which is right only while no
lane move feeds its scalar operands."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED_LANE_MOVES_IN_LOOP = 0   # profiles/fwd_production.md (the parent had 66)


def test_default_forward_keeps_its_registers_and_has_no_lane_spills_in_the_loop():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_census.py"), "--json"], check=True,
                         capture_output=True, text=True).stdout
    c = json.loads(out)
    assert "fwd_mfma_stag_kernel" in c["kernel"]
    assert c["loop_mfma"] == 64, "the census did not find the key-tile loop (64 MFMAs a trip)"
    assert c["scratch"] == 0
    assert c["vgpr"] <= 256
    assert c["lane_moves"] <= SHIPPED_LANE_MOVES_IN_LOOP
