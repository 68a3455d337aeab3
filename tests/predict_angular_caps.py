"""Grid cap of the angular prediction kernel -- a helper, not a test.

  launch_predict_angular (vvc-mip-gpu_amd/csrc/mip_predict_angular.hip): grid = min(ceil(n / 256), 1024)
      workgroups of 4 waves; a wave scans 64 consecutive list entries per pass, one per lane (row r
      of the list = entries 64 r .. 64 r + 63), and emits the angular items among them before it
      moves on: one round of the capped grid is 262 144 entries, independent of the CU count, and a
      wave's consecutive passes are the rows r and r + 4096.

tests/test_gpu_predict_angular.py sizes its multi-pass list from these constants;
tests/test_predict_angular_cpu.py reads the launcher's and the kernel's text and fails when a
constant here no longer is theirs.
"""
from launch_caps import CSRC, kernel_body, launcher_body, multipass_work, passes  # noqa: F401  (shared readers)

SOURCE = "mip_predict_angular.hip"
LAUNCHER = "launch_predict_angular"
KERNEL = "angular_predict_kernel"

WAVES = 4                        # kAngPredWaves
ENTRIES_PER_WAVE = 64            # kAngPredEntriesPerWave
GROUPS_CAP = 1024                # kAngPredGroupsCap: workgroups, whatever the device
ENTRIES_PER_ROUND = GROUPS_CAP * WAVES * ENTRIES_PER_WAVE     # 262 144
ROWS_PER_ROUND = GROUPS_CAP * WAVES                           # a wave's passes are rows r, r + 4096, ...
