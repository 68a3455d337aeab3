"""Grid cap of the angular prediction kernels -- a helper, not a test.

  launch_angular_predict (vvc-mip-gpu_amd/csrc/mip_predict_angular.hip), the one launch that
      launch_predict_angular, launch_predict_angular_ext and launch_predict_angular_tap4 go through:
      grid = min(ceil(n / 256), 1024) workgroups of 4 waves; a wave scans 64 consecutive list entries
      per pass, one per lane (row r of the list = entries 64 r .. 64 r + 63), and emits the angular
      items among them before it moves on: one round of the capped grid is 262 144 entries,
      independent of the CU count, and a wave's consecutive passes are the rows r and r + 4096.

tests/test_gpu_predict_angular.py sizes its multi-pass list from these constants;
tests/test_predict_angular_cpu.py reads the launch's and the kernels' text and fails when a
constant here no longer is theirs.
"""
from launch_caps import CSRC, kernel_body, launcher_body, launcher_function, multipass_work, passes, wrapped_body  # noqa: F401  (shared readers)

SOURCE = "mip_predict_angular.hip"
LAUNCH_RULE = "launch_angular_predict"      # the shared launch: argument rules, grid rule, the one hipLaunchKernelGGL
# (launcher, its kernel, what it hands the shared launch as "the length table is there")
LAUNCHERS = (("launch_predict_angular", "angular_predict_kernel", "true"),
             ("launch_predict_angular_ext", "angular_ext_predict_kernel", "a.ext != nullptr"),
             ("launch_predict_angular_tap4", "angular_tap4_predict_kernel", "true"))
LAUNCHER, KERNEL = LAUNCHERS[0][:2]
BODY = "angular_predict_items"              # the body all three kernels wrap

WAVES = 4                        # kAngPredWaves
ENTRIES_PER_WAVE = 64            # kAngPredEntriesPerWave
GROUPS_CAP = 1024                # kAngPredGroupsCap: workgroups, whatever the device
ENTRIES_PER_ROUND = GROUPS_CAP * WAVES * ENTRIES_PER_WAVE     # 262 144
ROWS_PER_ROUND = GROUPS_CAP * WAVES                           # a wave's passes are rows r, r + 4096, ...
