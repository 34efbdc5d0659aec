"""-m gpu: the five launchers whose dynamic LDS can exceed the 64 KiB default (csrc/host_launch.h, launch_big_lds), each driven
small -> large -> small in ONE fresh process, so the large call is the one that has to raise the kernel's limit and the second small
call runs under the raised limit.  Every call is judged by the op's own GPU test (its comparison, its tolerance, its LAST_PATH
assertion); the child calls those test functions.  With a second GPU the large shapes run again there: the raised limit is kept
per (kernel instantiation, device), and a process-wide record would skip the set on the second device.

Shapes, from each file's own size function (B = H = 1; bytes of dynamic LDS):
  fused Edgewise forward   FusedCfg<NT, 64>::lds_bytes(V)   N = 64, V = 8 (NT = 2): 54,176    N = 65, V = 5 (NT = 3): 74,016
  fused Edgewise backward  BwdCfg<NT, 64>::lds_bytes(V)     N = 64, V = 8         : 51,648    N = 65, V = 5         : 70,336
  lens means forward       lm_smem_bytes<64>                N = 24, L V = 1 x 2: 11,520    N = 121, L V = 4 x 4: 65,568
  lens means backward      lm_smem_bytes<64>, bwd           N = 24, L V = 1 x 2: 16,576    N = 121, L V = 4 x 4: 113,184
  alignment_cost           ac_lds_bytes(N, 7) = (70 N + 1168) 4   N = 100: 32,672    N = 218: 65,712   (N = 217: 65,432)
  log_mel                  lm_lds_bytes(n_fft) = (34 n_fft + 32) 4   n_fft = 400: 54,528    n_fft = 482: 65,680   (480: 65,408)
N = 65 is the first sequence length of the fused pair above 64 KiB at dk = 64 (NT changes at multiples of 32, and the size depends
on (NT, dk, V) only: NT = 2 stays below 64 KiB up to V = 8, NT = 3 is above it from V = 2 on, so the pair's small and large calls
are two instantiations, where the other three launchers cross inside one: no dk = 64 shape of the pair stays under 64 KiB inside an
instantiation that can exceed it, so for the pair the second small call does not run under a raised limit).  The small shape is a case of the pair's own sweep
(test_fused_vs_oracle_shape_sweep).  N = 121 is the first for the lens forward at its 16 channels; 218 and 482 are the first for
the two Whisper kernels.

lens_means_hip has no fall-back to take (a refusal raises), so it records no LAST_PATH; the other four assert PATH_FUSED inside the
functions called here.  On one GPU this file would pass on a library that keeps the record per process: only the second-device
half tells the two apart, and its skip message says that it did not run.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

EW_SMALL, EW_LARGE = (1, 64, 64, 1, 8, 4), (1, 65, 64, 1, 5, 4)                    # B, N, D, H, V, r
LENS_SMALL, LENS_LARGE = (1, 24, 1, 64, 2, (1,)), (1, 121, 1, 64, 4, (1, 2, 3, 4))  # B, N, H, dk, V, dilations
AC_SMALL, AC_LARGE, AC_WIDTH = 100, 218, 7
LM_SMALL, LM_LARGE = (400, 160, 80), (482, 160, 80)                                # n_fft, hop, n_mels


def _edgewise(shape):
    import mop_amd
    from mop_amd import ops
    from test_gpu_edgewise import test_fused_vs_oracle_shape_sweep
    try:
        test_fused_vs_oracle_shape_sweep(shape)          # forward and backward, LAST_PATH of both
    finally:
        mop_amd.set_precision("auto")
        ops.set_path("auto")


def _lens(shape):
    import torch
    from test_gpu_edgewise import test_lens_means_kernels_vs_torch_statement
    for dtype in (torch.bfloat16, torch.float32):         # two instantiations, each with a limit of its own
        test_lens_means_kernels_vs_torch_statement(shape, dtype)


def _align(N):
    from test_gpu_whisper_align import _cost_both
    from test_whisper_align_cpu import cost_case
    probs, nt, nf = cost_case(2, N, 9, [N], [9], N, "cuda")
    _cost_both(probs, nt, nf, AC_WIDTH, f"N = {N}")


def _log_mel(shape):
    from test_gpu_whisper_frontend import check
    from test_whisper_frontend_cpu import noise
    n_fft, hop, _ = shape
    return check([noise(hop * 40 + 7, seed=n_fft)], shape, "broadband", f"n_fft = {n_fft}")


LAUNCHERS = [("edgewise fused fwd+bwd", _edgewise, EW_SMALL, EW_LARGE), ("lens means fwd+bwd", _lens, LENS_SMALL, LENS_LARGE),
             ("alignment_cost", _align, AC_SMALL, AC_LARGE), ("log_mel", _log_mel, LM_SMALL, LM_LARGE)]


def child():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name, run, small, large in LAUNCHERS:
        first = run(small)
        run(large)
        again = run(small)
        if first is not None:
            assert torch.equal(first, again), name       # log_mel is bitwise reproducible
        print(f"device 0: {name} small, large, small ok", flush=True)
    print("DEVICE0 OK", flush=True)
    if torch.cuda.device_count() < 2:
        print("DEVICE1 ABSENT", flush=True)
        return
    torch.cuda.set_device(1)
    for name, run, _, large in LAUNCHERS:
        run(large)
        print(f"device 1: {name} large ok", flush=True)
    print("DEVICE1 OK", flush=True)


@pytest.fixture(scope="module")
def child_output():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_small_large_small_in_one_process(child_output):
    assert child_output.returncode == 0, child_output.stderr[-2000:]
    assert "DEVICE0 OK" in child_output.stdout


def test_large_shapes_on_a_second_device(child_output):
    if "DEVICE1 ABSENT" in child_output.stdout:
        pytest.skip("one GPU: the large shapes were not run on a second device, so the per-device record of the raised LDS limit "
                    "was exercised on device 0 only")
    assert child_output.returncode == 0 and "DEVICE1 OK" in child_output.stdout, child_output.stderr[-2000:]


if __name__ == "__main__":
    child()
