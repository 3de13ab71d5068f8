"""Launch shapes at which the head (input staging) and the tail (wave-cooperative copy-out) of the forward-dynamics-gradient kernel can go wrong, and how to
run them.  Shared by tests/test_gpu_kernel_shell.py, tests/test_kernel_shell_emulation.py and tools/make_shell_golden.py (which recorded
tests/golden/kernel_shell/parent_<robot>.npz from the build before include/grid_kernel_shell.h existed).  Not a test module."""
import numpy as np

SEED = 20
N_MAX = 65
# name: (N, blocks, threads, input stride - 3n, input offset in elements, output offset in elements); blocks / threads 0 = the library's default
CASES = {
    "n1": (1, 0, 0, 0, 0, 0),
    "n7": (7, 0, 0, 0, 0, 0),
    "n8": (8, 0, 0, 0, 0, 0),          # one wave holds 8 solves of a 7-joint arm
    "n9": (9, 0, 0, 0, 0, 0),
    "n31": (31, 0, 0, 0, 0, 0),
    "n32": (32, 0, 0, 0, 0, 0),        # one 256-thread block holds 32
    "n33": (33, 0, 0, 0, 0, 0),
    "n65_one_block": (65, 1, 256, 0, 0, 0),   # grid-stride: three trips, ragged last
    "n40_t16": (40, 0, 16, 0, 0, 0),
    "n40_t64": (40, 0, 64, 0, 0, 0),
    "n33_stride_plus3": (33, 0, 0, 3, 0, 0),  # rows of 3n + 3 values (7-joint arm: 24)
    "n33_in_offset": (33, 0, 0, 0, 1, 0),     # input base 4 bytes past a 16-byte boundary
    "n33_out_offset": (33, 0, 0, 0, 0, 1),    # output base 4 bytes past a 16-byte boundary
}


def inputs(n):
    """The N_MAX states every case takes its first N rows from."""
    rng = np.random.default_rng(SEED)
    return np.hstack([rng.uniform(-np.pi, np.pi, (N_MAX, n)), rng.uniform(-2, 2, (N_MAX, n)), rng.uniform(-10, 10, (N_MAX, n))]).astype(np.float32)


def run_case(torch, lib, x, case):
    """Runs one case through the device entry point; torch None: lib is a CPU emulation build and the buffers are NumPy arrays.  Returns
    (records (N, 2n^2), guard): the output buffer is NaN-prefilled and has 2n^2 guard values behind the last record (and one in front of an offset
    base), which the kernel must leave alone; guard is what they hold afterwards."""
    N, blocks, threads, extra, in_off, out_off = CASES[case]
    n = lib.n
    rec = 2 * n * n
    stride = 3 * n + extra
    rows = np.zeros((N, stride), dtype=np.float32)
    rows[:, :3 * n] = x[:N]
    flat = np.concatenate([np.full(in_off, np.nan, dtype=np.float32), rows.reshape(-1)])
    lib.set_launch_dims(blocks, threads)
    try:
        if torch is None:
            out = np.full(out_off + N * rec + rec, np.nan, dtype=np.float32)
            lib.forward_dynamics_gradient_device(flat[in_off:], N, out[out_off:], stride=stride)
        else:
            d_in = torch.from_numpy(flat).cuda()
            d_out = torch.full((out_off + N * rec + rec,), float("nan"), dtype=torch.float32, device="cuda")
            assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0  # (the offset views below then start 4 bytes past a 16-byte boundary)
            lib.forward_dynamics_gradient_device(d_in[in_off:], N, d_out[out_off:], stride=stride, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
    finally:
        lib.set_launch_dims(0, 0)
    return out[out_off:out_off + N * rec].reshape(N, rec).copy(), np.concatenate([out[:out_off], out[out_off + N * rec:]])
