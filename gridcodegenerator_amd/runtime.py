"""Build + ctypes binding of the robot-specialised C-ABI library (include/grid_capi.h).

``build_library(robot)`` runs the generator, then hipcc for gfx950, and leaves ``libgrid_<robot>.so`` in-tree
(gridcodegenerator_amd/_build/<robot>/) so that it travels with the repository snapshot.  ``GridLibrary`` loads it.
There is no CPU fallback: if the library is missing or does not load, GridLibrary raises.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from .GRiDCodeGenerator import GRiDCodeGenerator
from .robot import RobotModel

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
BUILD_DIR = os.path.join(PKG_DIR, "_build")
CAPI_SRC = os.path.join(PKG_DIR, "csrc", "grid_capi.hip")
INCLUDE_DIR = os.path.join(REPO_DIR, "include")

# -fno-slp-vectorize: the SLP vectorizer pairs the unrolled 6-vector arithmetic into v_pk_*_f32, which on gfx950 has the
# same FLOP rate as scalar v_fma_f32 but needs even-aligned register pairs, extra v_mov shuffles and constants held in
# VGPR pairs (measured: +60 VGPRs and scratch spills in the RNEA kernel).
# -fno-signed-zeros -ffinite-math-only: lets the compiler fold the structural zeros of root-link vectors (0*x, x+0); no
# reassociation is enabled, results for finite inputs are unchanged except for the sign of exact zeros (-8.6 % VALU instructions).
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fno-signed-zeros", "-ffinite-math-only",
               "-shared", "-fPIC", "-Wno-unused-value",
               "-mllvm", "-amdgpu-kernarg-preload-count=8"]  # kernel arguments arrive in SGPRs with the dispatch (no s_load at the head of every wave): -0.15 us per launch


def library_path(robot_name, build_dir=None):
    return os.path.join(build_dir or BUILD_DIR, robot_name, "libgrid_%s.so" % robot_name)


def generate_header(robot, out_dir, namespace="grid", cols_per_lane=None, tuning=None, debug_mode=False):
    """Runs GRiDCodeGenerator(robot).gen_all_code() with out_dir as the working directory (the generator writes
    <namespace>.cuh into the cwd, like the reference does)."""
    os.makedirs(out_dir, exist_ok=True)
    cwd = os.getcwd()
    os.chdir(out_dir)
    try:
        GRiDCodeGenerator(robot, DEBUG_MODE=debug_mode, FILE_NAMESPACE=namespace, COLS_PER_LANE=cols_per_lane, tuning=tuning).gen_all_code()
    finally:
        os.chdir(cwd)
    return os.path.join(out_dir, namespace + ".cuh")


def build_library(robot, build_dir=None, force=False, extra_flags=(), verbose=False, cols_per_lane=None, tuning=None):
    """robot: a fixture name, a RobotModel, or any URDFParser-style robot object.  Returns the .so path.
    tuning: generation-time knobs (GRiDCodeGenerator.TUNING_DEFAULTS); nothing is read from the environment."""
    if isinstance(robot, str):
        robot = RobotModel.from_fixture(robot)
    name = robot.name
    out_dir = os.path.join(build_dir or BUILD_DIR, name)
    so = library_path(name, build_dir)
    header = generate_header(robot, out_dir, cols_per_lane=cols_per_lane, tuning=tuning)
    stamp = so + ".stamp"
    sig = open(header).read() + open(os.path.join(INCLUDE_DIR, "grid_kernel_shell.h")).read() + open(CAPI_SRC).read() + " ".join(HIPCC_FLAGS + list(extra_flags))
    import hashlib
    digest = hashlib.sha256(sig.encode()).hexdigest()
    if not force and os.path.exists(so) and os.path.exists(stamp) and open(stamp).read() == digest:
        return so
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc] + HIPCC_FLAGS + list(extra_flags) + ["-I" + out_dir, "-I" + INCLUDE_DIR, '-DGRID_ROBOT_NAME="%s"' % name, CAPI_SRC, "-o", so]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(digest)
    return so


_c_float_p = ctypes.POINTER(ctypes.c_float)


def _ptr(x):
    """Accepts a raw device/host address (int), a numpy float32 array, or anything with data_ptr() (torch tensors)."""
    if x is None:
        return ctypes.c_void_p(None)
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return ctypes.c_void_p(x.data_ptr())
    if isinstance(x, np.ndarray):
        if x.dtype != np.float32 or not x.flags["C_CONTIGUOUS"]:
            raise TypeError("expected a C-contiguous float32 array")
        return ctypes.c_void_p(x.ctypes.data)
    raise TypeError("cannot interpret %r as a pointer" % type(x))


class GridError(RuntimeError):
    pass


class GridLibrary:
    """Thin ctypes mirror of include/grid_capi.h for one robot."""

    def __init__(self, path, device=0, max_timesteps=16384):
        if not os.path.exists(path):
            raise GridError("robot library %s is missing - run gridcodegenerator_amd.runtime.build_library() / __graft_entry__.build(); "
                            "there is no CPU fallback" % path)
        self.path = path
        self.lib = ctypes.CDLL(path)
        L = self.lib
        if not hasattr(L, "grid_second_order_capacity"):
            raise GridError("%s was built from an older grid_capi.hip - rebuild it (gridcodegenerator_amd.runtime.build_library)" % path)
        L.grid_robot_name.restype = ctypes.c_char_p
        L.grid_last_error.restype = ctypes.c_char_p
        self.n = L.grid_num_joints()
        self.robot_name = L.grid_robot_name().decode()
        self.lanes_per_solve = L.grid_lanes_per_solve()
        self.suggested_threads = L.grid_suggested_threads()
        self.lds_bytes_per_block = L.grid_lds_bytes_per_block()
        self.has_second_order = bool(L.grid_has_second_order())
        self.handle = ctypes.c_void_p()
        self._check(L.grid_init(ctypes.c_int(device), ctypes.c_int(max_timesteps), ctypes.byref(self.handle)))
        self.max_timesteps = max_timesteps

    def pinned_empty(self, shape, dtype=np.float32):
        """A NumPy array in page-locked host memory (grid_host_alloc): with such buffers forward_dynamics_gradient_host(..., out=...) overlaps its copies
        with the kernel.  The memory is released when the array (and every view of it) is gone."""
        import weakref

        dtype = np.dtype(dtype)
        count = int(np.prod(shape))
        p = ctypes.c_void_p()
        self._check(self.lib.grid_host_alloc(ctypes.c_size_t(max(1, count * dtype.itemsize)), ctypes.byref(p)))
        buf = (ctypes.c_char * max(1, count * dtype.itemsize)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)
        weakref.finalize(buf, self.lib.grid_host_free, ctypes.c_void_p(p.value))
        return arr

    def second_order_capacity(self, f64=False):
        """Solves per call the second-order entry points accept on this handle (their buffers are capped at 1 GiB each)."""
        return self.lib.grid_second_order_capacity(self.handle, ctypes.c_int(1 if f64 else 0))

    def _check(self, rc):
        if rc != 0:
            raise GridError("%s (code %d)" % (self.lib.grid_last_error().decode(), rc))

    def close(self):
        if self.handle:
            self._check(self.lib.grid_close(self.handle))
            self.handle = ctypes.c_void_p()

    def set_launch_dims(self, blocks=0, threads=0):
        self._check(self.lib.grid_set_launch_dims(self.handle, ctypes.c_int(blocks), ctypes.c_int(threads)))

    # ---- host-buffer entry points (H2D, launch, D2H, synchronous): NumPy arrays in, NumPy arrays out
    def _host_in(self, a, cols, what, dtype=np.float32):
        x = np.ascontiguousarray(a, dtype=dtype)
        if x.ndim != 2 or x.shape[1] not in (cols if isinstance(cols, tuple) else (cols,)):
            raise ValueError("%s must have shape (N, %s)" % (what, cols))
        return x

    def forward_dynamics_gradient_host(self, q_qd_u, gravity=9.81, out=None):
        """out: optional (N, 2n^2) float32 result array (e.g. from pinned_empty(): with page-locked input AND output the C entry point pipelines its copies)."""
        x = q_qd_u if (isinstance(q_qd_u, np.ndarray) and q_qd_u.dtype == np.float32 and q_qd_u.flags["C_CONTIGUOUS"] and q_qd_u.ndim == 2 and q_qd_u.shape[1] == 3 * self.n) \
            else self._host_in(q_qd_u, 3 * self.n, "q_qd_u")  # (no copy of an array that already has the right layout: a copy would leave page-locked memory)
        N = x.shape[0]
        if out is None:
            out = np.empty((N, 2 * self.n * self.n), dtype=np.float32)
        elif out.dtype != np.float32 or out.shape != (N, 2 * self.n * self.n) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous float32 array of shape (N, 2n^2)")
        self._check(self.lib.grid_forward_dynamics_gradient_host(self.handle, _ptr(x), ctypes.c_int(N), ctypes.c_float(gravity), _ptr(out)))
        return out

    def forward_dynamics_gradient_host_f64(self, q_qd_u, gravity=9.81):
        x = self._host_in(q_qd_u, 3 * self.n, "q_qd_u", np.float64)
        N = x.shape[0]
        out = np.empty((N, 2 * self.n * self.n), dtype=np.float64)
        self._check(self.lib.grid_forward_dynamics_gradient_host_f64(self.handle, ctypes.c_void_p(x.ctypes.data), ctypes.c_int(N), ctypes.c_double(gravity),
                                                                     ctypes.c_void_p(out.ctypes.data)))
        return out

    def host_f64(self, algorithm, *arrays, gravity=9.81):
        """T = double host-buffer entry points: algorithm in {inverse_dynamics, inverse_dynamics_gradient, direct_minv, forward_dynamics, aba,
        idsva_so, fdsva_so, end_effector_pose, end_effector_pose_gradient, end_effector_pose_gradient_hessian, crba}; arrays as for the float methods
        (q_qd[, qdd] / q / q_qd_u[, qdd]) in float64."""
        n = self.n
        if algorithm in ("end_effector_pose", "end_effector_pose_gradient", "end_effector_pose_gradient_hessian"):
            return self._ee_host(("end_effector_pose", "end_effector_pose_gradient", "end_effector_pose_gradient_hessian").index(algorithm), arrays[0], np.float64)
        if algorithm == "crba":
            return self._crba_host(arrays[0], np.float64)
        P = lambda a: ctypes.c_void_p(None) if a is None else ctypes.c_void_p(a.ctypes.data)
        # same column rules as the float methods; entry points without a stride argument read exactly 3n values per solve
        first = {"inverse_dynamics": (2 * n, 3 * n), "inverse_dynamics_gradient": (2 * n, 3 * n), "direct_minv": (n, 2 * n, 3 * n)}.get(algorithm, 3 * n)
        a0 = self._host_in(arrays[0], first, "first input of " + algorithm, np.float64)
        N = a0.shape[0]

        def D(a):
            if a is None:
                return None
            x = self._host_in(a, n, "qdd", np.float64)
            if x.shape[0] != N:
                raise ValueError("qdd must have as many rows as the first input")
            return x
        cols = {"inverse_dynamics": n, "inverse_dynamics_gradient": 2 * n * n, "direct_minv": n * n, "forward_dynamics": n, "aba": n,
                "idsva_so": 4 * n ** 3, "fdsva_so": 4 * n ** 3}[algorithm]
        out = np.empty((N, cols), dtype=np.float64)
        fn = getattr(self.lib, "grid_%s_host_f64" % algorithm)
        g = ctypes.c_double(gravity)
        if algorithm in ("inverse_dynamics", "inverse_dynamics_gradient"):
            qdd = D(arrays[1]) if len(arrays) > 1 else None
            rc = fn(self.handle, P(a0), ctypes.c_int(a0.shape[1]), P(qdd), ctypes.c_int(N), g, P(out))
        elif algorithm == "direct_minv":
            rc = fn(self.handle, P(a0), ctypes.c_int(a0.shape[1]), ctypes.c_int(N), P(out))
        elif algorithm == "idsva_so":
            qdd = D(arrays[1]) if len(arrays) > 1 else None
            rc = fn(self.handle, P(a0), P(qdd), ctypes.c_int(N), g, P(out))
        else:
            rc = fn(self.handle, P(a0), ctypes.c_int(N), g, P(out))
        self._check(rc)
        return out

    def forward_dynamics_gradient_qdd_minv_host(self, q_qd, qdd, Minv, gravity=9.81):
        n = self.n
        x = self._host_in(q_qd, (2 * n, 3 * n), "q_qd")
        N = x.shape[0]
        a, M = self._host_in(qdd, n, "qdd"), self._host_in(Minv, n * n, "Minv")
        out = np.empty((N, 2 * n * n), dtype=np.float32)
        self._check(self.lib.grid_forward_dynamics_gradient_qdd_minv_host(self.handle, _ptr(x), ctypes.c_int(x.shape[1]), _ptr(a), _ptr(M), ctypes.c_int(N),
                                                                          ctypes.c_float(gravity), _ptr(out)))
        return out

    def inverse_dynamics_host(self, q_qd, qdd=None, gravity=9.81):
        n = self.n
        x = self._host_in(q_qd, (2 * n, 3 * n), "q_qd")
        a = None if qdd is None else self._host_in(qdd, n, "qdd")
        out = np.empty((x.shape[0], n), dtype=np.float32)
        self._check(self.lib.grid_inverse_dynamics_host(self.handle, _ptr(x), ctypes.c_int(x.shape[1]), _ptr(a), ctypes.c_int(x.shape[0]), ctypes.c_float(gravity), _ptr(out)))
        return out

    def inverse_dynamics_gradient_host(self, q_qd, qdd=None, gravity=9.81):
        n = self.n
        x = self._host_in(q_qd, (2 * n, 3 * n), "q_qd")
        a = None if qdd is None else self._host_in(qdd, n, "qdd")
        out = np.empty((x.shape[0], 2 * n * n), dtype=np.float32)
        self._check(self.lib.grid_inverse_dynamics_gradient_host(self.handle, _ptr(x), ctypes.c_int(x.shape[1]), _ptr(a), ctypes.c_int(x.shape[0]), ctypes.c_float(gravity), _ptr(out)))
        return out

    def direct_minv_host(self, q):
        n = self.n
        x = self._host_in(q, (n, 2 * n, 3 * n), "q")
        out = np.empty((x.shape[0], n * n), dtype=np.float32)
        self._check(self.lib.grid_direct_minv_host(self.handle, _ptr(x), ctypes.c_int(x.shape[1]), ctypes.c_int(x.shape[0]), _ptr(out)))
        return out

    # ---- joint-space inertia matrix: (N, n | 2n | 3n) rows whose first n values are q -> (N, n*n) dense symmetric M
    def _crba_host(self, q, dtype):
        n = self.n
        x = self._host_in(q, (n, 2 * n, 3 * n), "q", dtype)
        out = np.empty((x.shape[0], n * n), dtype=dtype)
        fn = self.lib.grid_crba_host_f64 if dtype == np.float64 else self.lib.grid_crba_host
        self._check(fn(self.handle, ctypes.c_void_p(x.ctypes.data), ctypes.c_int(x.shape[1]), ctypes.c_int(x.shape[0]), ctypes.c_void_p(out.ctypes.data)))
        return out

    def crba_host(self, q):
        return self._crba_host(q, np.float32)

    # ---- the rollout family: what its entry points share
    def _typed(self, name, f64):
        """(ctypes type of a real argument, entry point `name` of the library) in double or single precision"""
        return (ctypes.c_double, getattr(self.lib, name + "_f64")) if f64 else (ctypes.c_float, getattr(self.lib, name))

    def _u_strides(self, N, shared):
        """(stride_u_step, stride_u_solve) of a dense control (T, N, n), or of ONE sequence (T, n) shared by all solves"""
        return (self.n, 0) if shared else (N * self.n, self.n)

    def _u_layout(self, u, N, dtype=None, T=None):
        """(uu, T, stride_u_step, stride_u_solve) of a control of shape (T, N, n), or (T, n) shared by all solves.  dtype: u becomes a C-contiguous NumPy array
        of it (None: u, e.g. a torch tensor, is taken as it is); T: the number of steps u must have (the adjoint knows it from traj)."""
        n = self.n
        uu = u if dtype is None else np.ascontiguousarray(u, dtype=dtype)
        shared = uu.ndim == 2
        if tuple(uu.shape[1:]) != ((n,) if shared else (N, n)) or (T is not None and uu.shape[0] != T):
            raise ValueError("u must have shape (T, N, n) or (T, n) with %sN = %d, n = %d" % ("" if T is None else "T = %d, " % T, N, n))
        return (uu, uu.shape[0]) + self._u_strides(N, shared)

    def _rollout_forward_host(self, name, x0, u, dt, gravity, dtype, want, outputs):
        """The host entry point `name` of rollout / rollout_linearized; outputs: what it can write, in the order of its arguments; want: what it is asked for."""
        n = self.n
        x = self._host_in(x0, (2 * n, 3 * n), "x0", dtype)
        N = x.shape[0]
        uu, T, stride_step, stride_solve = self._u_layout(u, N, dtype)
        shapes = {"traj": (T + 1, N, 2 * n), "xT": (N, 2 * n), "fx": (T, N, 2 * n * n), "fu": (T, N, n * n)}
        out = {k: np.empty(shapes[k], dtype=dtype) for k in want}
        real, fn = self._typed(name, dtype == np.float64)
        self._check(fn(self.handle, ctypes.c_void_p(x.ctypes.data), ctypes.c_int(x.shape[1]), ctypes.c_void_p(uu.ctypes.data if uu.size else None), ctypes.c_long(stride_step),
                       ctypes.c_int(stride_solve), ctypes.c_int(N), ctypes.c_int(T), real(dt), real(gravity), *[ctypes.c_void_p(out[k].ctypes.data if k in out else None) for k in outputs]))
        return tuple(out[k] for k in want)

    def _rollout_forward_device(self, fn, real, d_x0, stride_x0, d_u, N, T, dt, outputs, u_shared, gravity, stream):
        """The device entry point fn of rollout / rollout_linearized; outputs: its output arguments"""
        stride_step, stride_solve = self._u_strides(N, u_shared)
        self._check(fn(self.handle, _ptr(d_x0), ctypes.c_int(stride_x0 or 2 * self.n), _ptr(d_u), ctypes.c_long(stride_step), ctypes.c_int(stride_solve), ctypes.c_int(N), ctypes.c_int(T),
                       real(dt), real(gravity), *[_ptr(o) for o in outputs], ctypes.c_void_p(stream)))

    # ---- fused rollout: x0 (N, 2n | 3n) rows starting with [q | qd], u (T, N, n) or one shared sequence (T, n) -> traj (T+1, N, 2n) or xT (N, 2n)
    def _rollout_host(self, x0, u, dt, final_only, gravity, dtype):
        return self._rollout_forward_host("grid_rollout_host", x0, u, dt, gravity, dtype, ("xT",) if final_only else ("traj",), ("traj", "xT"))[0]

    def rollout_host(self, x0, u, dt, final_only=False, gravity=9.81):
        """T steps of ABA + semi-implicit Euler in one launch: the float32 trajectory (T+1, N, 2n) with row 0 = x0, or with final_only the last state (N, 2n)"""
        return self._rollout_host(x0, u, dt, final_only, gravity, np.float32)

    def rollout_host_f64(self, x0, u, dt, final_only=False, gravity=9.81):
        return self._rollout_host(x0, u, dt, final_only, gravity, np.float64)

    # ---- linearised rollout: the trajectory and, per step, fx = [d qdd/dq | d qdd/dqd] (df_du records) and fu = d qdd/du = M^-1 (dense, symmetric)
    def _rollout_linearized_host(self, x0, u, dt, gravity, dtype, want=("traj", "fx", "fu")):
        return self._rollout_forward_host("grid_rollout_linearized_host", x0, u, dt, gravity, dtype, want, ("traj", "xT", "fx", "fu"))

    def rollout_linearized_host(self, x0, u, dt, gravity=9.81, want=("traj", "fx", "fu")):
        """T steps of (forward dynamics gradient, M^-1, semi-implicit Euler) in one launch -> (traj (T+1, N, 2n), fx (T, N, 2n^2), fu (T, N, n^2)) in float32;
        x0, u as for rollout_host.  want: which of "traj", "xT", "fx", "fu" to compute and return, in that order (outputs left out cost no bandwidth;
        without "fu" the work only M^-1 needs is skipped)."""
        return self._rollout_linearized_host(x0, u, dt, gravity, np.float32, tuple(want))

    def rollout_linearized_host_f64(self, x0, u, dt, gravity=9.81, want=("traj", "fx", "fu")):
        return self._rollout_linearized_host(x0, u, dt, gravity, np.float64, tuple(want))

    # ---- rollout adjoint: gradient of a trajectory cost with respect to x0 and every u_t from the stored states, the controls and gx = d cost / d traj
    def _rollout_adjoint_host(self, traj, u, dt, gx, gxT, gravity, dtype, want):
        n = self.n
        tr = np.ascontiguousarray(traj, dtype=dtype)
        if tr.ndim != 3 or tr.shape[2] != 2 * n:
            raise ValueError("traj must have shape (T+1, N, 2n) with n = %d" % n)
        T, N = tr.shape[0] - 1, tr.shape[1]
        uu, _, stride_step, stride_solve = self._u_layout(u, N, dtype, T)
        want = tuple(want)
        if not want or any(k not in ("grad_x0", "grad_u") for k in want):
            raise ValueError('want must name "grad_x0" and / or "grad_u"')
        g = None if gx is None else np.ascontiguousarray(gx, dtype=dtype)
        gT = None if gxT is None else np.ascontiguousarray(gxT, dtype=dtype)
        if g is not None and g.shape != tr.shape:
            raise ValueError("gx must have the shape of traj")
        if gT is not None and gT.shape != (N, 2 * n):
            raise ValueError("gxT must have shape (N, 2n)")
        shapes = {"grad_x0": (N, 2 * n), "grad_u": (T, N, n)}
        out = {k: np.empty(shapes[k], dtype=dtype) for k in want}
        P = lambda a: ctypes.c_void_p(a.ctypes.data if a is not None and a.size else None)
        real, fn = self._typed("grid_rollout_adjoint_host", dtype == np.float64)
        self._check(fn(self.handle, P(tr), P(uu), ctypes.c_long(stride_step), ctypes.c_int(stride_solve), ctypes.c_int(N), ctypes.c_int(T), real(dt), real(gravity),
                       P(g), P(gT), P(out.get("grad_x0")), P(out.get("grad_u"))))
        return tuple(out[k] for k in want)

    def rollout_adjoint_host(self, traj, u, dt, gx=None, gxT=None, gravity=9.81, want=("grad_x0", "grad_u")):
        """The reverse pass of rollout in one launch -> (grad_x0 (N, 2n), grad_u (T, N, n)) in float32: the gradient of a cost L = sum_t l_t(x_t) with respect to
        x0 and every u_t.  traj (T+1, N, 2n) and u ((T, N, n), or (T, n) shared) are what rollout_host read and wrote; gx (T+1, N, 2n) = d L / d traj and / or
        gxT (N, 2n) = d L / d x_T (at least one; both add at step T).  want: which of "grad_x0", "grad_u" to compute and return, in that order (without "grad_u"
        the work only M^-1 needs is skipped).  grad_u is ALWAYS per solve: for a shared u the gradient with respect to the one sequence is grad_u.sum(axis=1)."""
        return self._rollout_adjoint_host(traj, u, dt, gx, gxT, gravity, np.float32, want)

    def rollout_adjoint_host_f64(self, traj, u, dt, gx=None, gxT=None, gravity=9.81, want=("grad_x0", "grad_u")):
        return self._rollout_adjoint_host(traj, u, dt, gx, gxT, gravity, np.float64, want)

    # ---- closed-loop rollout: u_t = clamp(u_ff_t + K_t (x_t - x_ref_t)) formed inside the fused step loop
    def _feedback_layout(self, a, what, rec, N, T, dtype):
        """(array, stride_step, stride_solve) of K (rec = 2n^2) or x_ref (rec = 2n): (>= T, N, rec) dense, (>= T, rec) shared by all solves, (rec,) one record for everything"""
        aa = np.ascontiguousarray(a, dtype=dtype)
        if aa.ndim == 3 and aa.shape[0] >= T and tuple(aa.shape[1:]) == (N, rec):
            return aa, N * rec, rec
        if aa.ndim == 2 and aa.shape[0] >= T and aa.shape[1] == rec:
            return aa, rec, 0
        if aa.ndim == 1 and aa.shape[0] == rec:
            return aa, 0, 0
        raise ValueError("%s must have shape (T, N, %d), (T, %d) or (%d,) with T %s %d, N = %d" % (what, rec, rec, rec, "=" if what == "K" else ">=", T, N))

    def _rollout_feedback_host(self, x0, u_ff, K, x_ref, dt, u_min, u_max, want, gravity, dtype):
        n = self.n
        x = self._host_in(x0, (2 * n, 3 * n), "x0", dtype)
        N = x.shape[0]
        uu, T, su_step, su_solve = self._u_layout(u_ff, N, dtype)
        KK, sK_step, sK_solve = self._feedback_layout(K, "K", 2 * n * n, N, T, dtype)
        if KK.ndim > 1 and KK.shape[0] != T:
            raise ValueError("K must have as many steps as u_ff (%d)" % T)
        xr, sx_step, sx_solve = self._feedback_layout(x_ref, "x_ref", 2 * n, N, T, dtype)
        if (u_min is None) != (u_max is None):
            raise ValueError("u_min and u_max come together")
        lim = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=dtype), (n,))) for a in (u_min, u_max)]
        want = tuple(want)
        if not want or any(k not in ("traj", "xT", "u") for k in want):
            raise ValueError('want must name "traj", "xT" and / or "u"')
        shapes = {"traj": (T + 1, N, 2 * n), "xT": (N, 2 * n), "u": (T, N, n)}
        out = {k: np.empty(shapes[k], dtype=dtype) for k in want}
        P = lambda a: ctypes.c_void_p(a.ctypes.data if a is not None and a.size else None)
        real, fn = self._typed("grid_rollout_feedback_host", dtype == np.float64)
        self._check(fn(self.handle, P(x), ctypes.c_int(x.shape[1]), P(uu), ctypes.c_long(su_step), ctypes.c_int(su_solve), ctypes.c_int(N), ctypes.c_int(T), real(dt), real(gravity),
                       P(KK), ctypes.c_long(sK_step), ctypes.c_long(sK_solve), P(xr), ctypes.c_long(sx_step), ctypes.c_long(sx_solve), P(lim[0]), P(lim[1]),
                       P(out.get("traj")), P(out.get("xT")), P(out.get("u"))))
        return tuple(out[k] for k in want)

    def rollout_feedback_host(self, x0, u_ff, K, x_ref, dt, u_min=None, u_max=None, want=("traj", "u"), gravity=9.81):
        """T closed-loop steps in one launch -> (traj (T+1, N, 2n), u_applied (T, N, n)) in float32.  Per step u = clamp(u_ff + K (x - x_ref)), then ABA + semi-implicit
        Euler as rollout_host.  x0, u_ff as x0, u of rollout_host; K (T, N, 2n^2) records K[c*n + j] (gain_records makes them), (T, 2n^2) shared by all solves, or (2n^2,) one
        gain for everything; x_ref (>= T, N, 2n) (a nominal traj passes as it is), (>= T, 2n) shared by all solves, or (2n,) a set point; u_min, u_max: (n,) or scalars,
        both or neither.  want: which of "traj", "xT", "u" to compute and return, in that order."""
        return self._rollout_feedback_host(x0, u_ff, K, x_ref, dt, u_min, u_max, want, gravity, np.float32)

    def rollout_feedback_host_f64(self, x0, u_ff, K, x_ref, dt, u_min=None, u_max=None, want=("traj", "u"), gravity=9.81):
        return self._rollout_feedback_host(x0, u_ff, K, x_ref, dt, u_min, u_max, want, gravity, np.float64)

    def forward_dynamics_host(self, q_qd_u, gravity=9.81, aba=False):
        x = self._host_in(q_qd_u, 3 * self.n, "q_qd_u")
        out = np.empty((x.shape[0], self.n), dtype=np.float32)
        fn = self.lib.grid_aba_host if aba else self.lib.grid_forward_dynamics_host
        self._check(fn(self.handle, _ptr(x), ctypes.c_int(x.shape[0]), ctypes.c_float(gravity), _ptr(out)))
        return out

    def idsva_so_host(self, q_qd_u, qdd=None, gravity=9.81):
        n = self.n
        x = self._host_in(q_qd_u, 3 * n, "q_qd_u")
        a = None if qdd is None else self._host_in(qdd, n, "qdd")
        out = np.empty((x.shape[0], 4 * n ** 3), dtype=np.float32)
        self._check(self.lib.grid_idsva_so_host(self.handle, _ptr(x), _ptr(a), ctypes.c_int(x.shape[0]), ctypes.c_float(gravity), _ptr(out)))
        return out

    def fdsva_so_host(self, q_qd_u, gravity=9.81):
        n = self.n
        x = self._host_in(q_qd_u, 3 * n, "q_qd_u")
        out = np.empty((x.shape[0], 4 * n ** 3), dtype=np.float32)
        self._check(self.lib.grid_fdsva_so_host(self.handle, _ptr(x), ctypes.c_int(x.shape[0]), ctypes.c_float(gravity), _ptr(out)))
        return out

    def forward_dynamics_gradient_single_timing(self, q_qd_u_one, reps, gravity=9.81):
        x = np.ascontiguousarray(q_qd_u_one, dtype=np.float32).reshape(3 * self.n)
        out = np.empty(2 * self.n * self.n, dtype=np.float32)
        us = ctypes.c_double()
        self._check(self.lib.grid_forward_dynamics_gradient_single_timing(self.handle, _ptr(x), ctypes.c_int(reps), ctypes.c_float(gravity), _ptr(out), ctypes.byref(us)))
        return out, us.value

    # ---- end-effector kinematics (every leaf joint is an end effector): pose (N, 6E), gradient (N, 6En), Hessian (N, 6En^2); q of width n or 3n
    @property
    def num_end_effectors(self):
        return self.lib.grid_num_end_effectors()

    @property
    def end_effector_joints(self):
        E = self.num_end_effectors
        out = (ctypes.c_int * E)()
        self._check(self.lib.grid_end_effector_joints(out))
        return list(out)

    def _ee_cols(self):
        n, E = self.n, self.num_end_effectors
        return 6 * E, 6 * E * n, 6 * E * n * n

    def _ee_host(self, which, q, dtype):
        x = self._host_in(q, (self.n, 3 * self.n), "q", dtype)
        N = x.shape[0]
        P = lambda a: ctypes.c_void_p(None) if a is None else ctypes.c_void_p(a.ctypes.data)
        sfx = "_f64" if dtype == np.float64 else ""
        out = np.empty((N, self._ee_cols()[which]), dtype=dtype)
        if which == 2:
            dee = np.empty((N, self._ee_cols()[1]), dtype=dtype)
            self._check(self.lib["grid_end_effector_pose_gradient_hessian_host" + sfx](self.handle, P(x), ctypes.c_int(x.shape[1]), ctypes.c_int(N), P(out), P(dee)))
            return out, dee
        fn = self.lib[("grid_end_effector_pose_host", "grid_end_effector_pose_gradient_host")[which] + sfx]
        self._check(fn(self.handle, P(x), ctypes.c_int(x.shape[1]), ctypes.c_int(N), P(out)))
        return out

    def end_effector_pose_host(self, q):
        return self._ee_host(0, q, np.float32)

    def end_effector_pose_gradient_host(self, q):
        return self._ee_host(1, q, np.float32)

    def end_effector_pose_gradient_hessian_host(self, q):
        """returns (d2eePos (N, 6En^2), deePos (N, 6En))"""
        return self._ee_host(2, q, np.float32)

    def end_effector_pose_device(self, d_q, N, d_eePos, stride=None, stream=0):
        self._check(self.lib.grid_end_effector_pose_device(self.handle, _ptr(d_q), ctypes.c_int(stride or self.n), ctypes.c_int(N), _ptr(d_eePos), ctypes.c_void_p(stream)))

    def end_effector_pose_gradient_device(self, d_q, N, d_deePos, stride=None, stream=0):
        self._check(self.lib.grid_end_effector_pose_gradient_device(self.handle, _ptr(d_q), ctypes.c_int(stride or self.n), ctypes.c_int(N), _ptr(d_deePos),
                                                                    ctypes.c_void_p(stream)))

    def end_effector_pose_gradient_hessian_device(self, d_q, N, d_d2eePos, d_deePos=None, stride=None, stream=0):
        self._check(self.lib.grid_end_effector_pose_gradient_hessian_device(self.handle, _ptr(d_q), ctypes.c_int(stride or self.n), ctypes.c_int(N), _ptr(d_d2eePos),
                                                                            _ptr(d_deePos), ctypes.c_void_p(stream)))

    # ---- device-pointer entry points (asynchronous on `stream`)
    def forward_dynamics_gradient_device(self, d_q_qd_u, N, d_df_du, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_forward_dynamics_gradient_device(self.handle, _ptr(d_q_qd_u), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N),
                                                                   ctypes.c_float(gravity), _ptr(d_df_du), ctypes.c_void_p(stream)))

    def prepare_forward_dynamics_gradient_device(self, d_q_qd_u, N, d_df_du, stride=None, gravity=9.81, stream=0):
        """Returns a zero-argument callable that enqueues the same launch every time it is called: the ctypes argument objects are built
        once, so a call costs one foreign-function call (an MPC loop re-launching on the same buffers; bench.py's step)."""
        fn = self.lib.grid_forward_dynamics_gradient_device
        args = (self.handle, _ptr(d_q_qd_u), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N), ctypes.c_float(gravity), _ptr(d_df_du), ctypes.c_void_p(stream))
        check = self._check

        def launch():
            rc = fn(*args)
            if rc:
                check(rc)
        return launch

    def forward_dynamics_gradient_device_f64(self, d_q_qd_u, N, d_df_du, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_forward_dynamics_gradient_device_f64(self.handle, _ptr(d_q_qd_u), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N),
                                                                       ctypes.c_double(gravity), _ptr(d_df_du), ctypes.c_void_p(stream)))

    def forward_dynamics_gradient_qdd_minv_device(self, d_q_qd, d_qdd, d_Minv, N, d_df_du, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_forward_dynamics_gradient_qdd_minv_device(self.handle, _ptr(d_q_qd), ctypes.c_int(stride or 3 * self.n), _ptr(d_qdd), _ptr(d_Minv),
                                                                            ctypes.c_int(N), ctypes.c_float(gravity), _ptr(d_df_du), ctypes.c_void_p(stream)))

    def inverse_dynamics_device(self, d_q_qd, d_qdd, N, d_c, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_inverse_dynamics_device(self.handle, _ptr(d_q_qd), ctypes.c_int(stride or 3 * self.n), _ptr(d_qdd), ctypes.c_int(N),
                                                          ctypes.c_float(gravity), _ptr(d_c), ctypes.c_void_p(stream)))

    def direct_minv_device(self, d_q, N, d_Minv, stride=None, stream=0):
        self._check(self.lib.grid_direct_minv_device(self.handle, _ptr(d_q), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N), _ptr(d_Minv), ctypes.c_void_p(stream)))

    def crba_device(self, d_q, N, d_M, stride=None, stream=0):
        """stride defaults to 3n (q_qd_u rows), as for direct_minv_device; the kernel reads the first n values of every row"""
        self._check(self.lib.grid_crba_device(self.handle, _ptr(d_q), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N), _ptr(d_M), ctypes.c_void_p(stream)))

    def rollout_device(self, d_x0, d_u, N, T, dt, d_traj=None, d_xT=None, stride_x0=None, u_shared=False, gravity=9.81, stream=0):
        """Asynchronous on `stream`, allocates nothing.  d_x0: rows of stride_x0 (default 2n) values starting with [q | qd]; d_u: dense (T, N, n), or with u_shared
        ONE sequence (T, n) for all solves; d_traj (T+1, N, 2n) and / or d_xT (N, 2n): at least one of them."""
        self._rollout_forward_device(self.lib.grid_rollout_device, ctypes.c_float, d_x0, stride_x0, d_u, N, T, dt, (d_traj, d_xT), u_shared, gravity, stream)

    def rollout_linearized_device(self, d_x0, d_u, N, T, dt, d_traj=None, d_xT=None, d_fx=None, d_fu=None, stride_x0=None, u_shared=False, gravity=9.81, stream=0):
        """Asynchronous on `stream`, allocates nothing.  Inputs as rollout_device; outputs (torch tensors or raw addresses, float32, each optional, at least one):
        d_traj (T+1, N, 2n), d_xT (N, 2n), d_fx (T, N, 2n^2), d_fu (T, N, n^2)."""
        self._rollout_forward_device(self.lib.grid_rollout_linearized_device, ctypes.c_float, d_x0, stride_x0, d_u, N, T, dt, (d_traj, d_xT, d_fx, d_fu), u_shared, gravity, stream)

    def _rollout_adjoint_device(self, fn, real, d_traj, d_u, N, T, dt, d_gx, d_gxT, d_grad_x0, d_grad_u, u_shared, gravity, stream):
        stride_step, stride_solve = self._u_strides(N, u_shared)
        self._check(fn(self.handle, _ptr(d_traj), _ptr(d_u), ctypes.c_long(stride_step), ctypes.c_int(stride_solve), ctypes.c_int(N), ctypes.c_int(T),
                       real(dt), real(gravity), _ptr(d_gx), _ptr(d_gxT), _ptr(d_grad_x0), _ptr(d_grad_u), ctypes.c_void_p(stream)))

    def rollout_adjoint_device(self, d_traj, d_u, N, T, dt, d_gx=None, d_gxT=None, d_grad_x0=None, d_grad_u=None, u_shared=False, gravity=9.81, stream=0):
        """Asynchronous on `stream`, allocates nothing.  d_traj (T+1, N, 2n) and d_u (dense (T, N, n), or with u_shared ONE sequence (T, n)) as rollout_device read
        and wrote them; cotangents d_gx (T+1, N, 2n) and / or d_gxT (N, 2n): at least one; outputs d_grad_x0 (N, 2n) and / or d_grad_u (T, N, n): at least one
        (torch tensors or raw addresses, float32).  d_grad_u is ALWAYS per solve: with u_shared the gradient of the one sequence is its sum over the solves."""
        self._rollout_adjoint_device(self.lib.grid_rollout_adjoint_device, ctypes.c_float, d_traj, d_u, N, T, dt, d_gx, d_gxT, d_grad_x0, d_grad_u, u_shared, gravity, stream)

    def rollout_adjoint_device_f64(self, d_traj, d_u, N, T, dt, d_gx=None, d_gxT=None, d_grad_x0=None, d_grad_u=None, u_shared=False, gravity=9.81, stream=0):
        self._rollout_adjoint_device(self.lib.grid_rollout_adjoint_device_f64, ctypes.c_double, d_traj, d_u, N, T, dt, d_gx, d_gxT, d_grad_x0, d_grad_u, u_shared, gravity, stream)

    def _rollout_feedback_device(self, f64, d_x0, d_uff, d_K, d_xref, N, T, dt, d_traj, d_xT, d_u_out, d_u_min, d_u_max, stride_x0, u_shared, K_strides, xref_strides, gravity, stream):
        n = self.n
        real, fn = self._typed("grid_rollout_feedback_device", f64)
        su_step, su_solve = self._u_strides(N, u_shared)
        sK_step, sK_solve = K_strides if K_strides is not None else (N * 2 * n * n, 2 * n * n)
        sx_step, sx_solve = xref_strides if xref_strides is not None else (N * 2 * n, 2 * n)
        self._check(fn(self.handle, _ptr(d_x0), ctypes.c_int(stride_x0 or 2 * n), _ptr(d_uff), ctypes.c_long(su_step), ctypes.c_int(su_solve), ctypes.c_int(N), ctypes.c_int(T),
                       real(dt), real(gravity), _ptr(d_K), ctypes.c_long(sK_step), ctypes.c_long(sK_solve), _ptr(d_xref), ctypes.c_long(sx_step), ctypes.c_long(sx_solve),
                       _ptr(d_u_min), _ptr(d_u_max), _ptr(d_traj), _ptr(d_xT), _ptr(d_u_out), ctypes.c_void_p(stream)))

    def rollout_feedback_device(self, d_x0, d_uff, d_K, d_xref, N, T, dt, d_traj=None, d_xT=None, d_u_out=None, d_u_min=None, d_u_max=None,
                                stride_x0=None, u_shared=False, K_strides=None, xref_strides=None, gravity=9.81, stream=0):
        """Asynchronous on `stream`, allocates nothing.  d_x0, d_uff as d_x0, d_u of rollout_device; d_K dense (T, N, 2n^2) records K[c*n + j], d_xref dense (>= T, N, 2n), or
        with K_strides / xref_strides = (step stride, solve stride) in elements, 0 sharing one record between the steps / the solves; d_u_min, d_u_max (n,), both or neither;
        outputs d_traj (T+1, N, 2n), d_xT (N, 2n), d_u_out (T, N, n): at least one (torch tensors or raw addresses, float32)."""
        self._rollout_feedback_device(False, d_x0, d_uff, d_K, d_xref, N, T, dt, d_traj, d_xT, d_u_out, d_u_min, d_u_max, stride_x0, u_shared, K_strides, xref_strides, gravity, stream)

    def rollout_feedback_device_f64(self, d_x0, d_uff, d_K, d_xref, N, T, dt, d_traj=None, d_xT=None, d_u_out=None, d_u_min=None, d_u_max=None,
                                    stride_x0=None, u_shared=False, K_strides=None, xref_strides=None, gravity=9.81, stream=0):
        self._rollout_feedback_device(True, d_x0, d_uff, d_K, d_xref, N, T, dt, d_traj, d_xT, d_u_out, d_u_min, d_u_max, stride_x0, u_shared, K_strides, xref_strides, gravity, stream)

    def rollout_torch(self, x0, u, dt, gravity=9.81):
        """Differentiable rollout on torch tensors: traj (T+1, N, 2n) = rollout(x0, u) with autograd support.  x0 (N, 2n); u (T, N, n), or (T, n) shared by all
        solves (its gradient is the sum of the per-solve gradients over N); float32 or float64, x0 and u on the same device.  CUDA tensors go through the device
        entry points on torch's current stream (no host synchronisation; the outputs are the only allocations), CPU tensors through the host entry points.
        Forward is rollout (ABA), backward is rollout_adjoint on the saved traj and u; only the gradients autograd asks for are computed.  First order only:
        differentiating the backward pass raises."""
        return _rollout_function()(self, float(dt), float(gravity), x0, u)

    def forward_dynamics_device(self, d_q_qd_u, N, d_qdd, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_forward_dynamics_device(self.handle, _ptr(d_q_qd_u), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N),
                                                          ctypes.c_float(gravity), _ptr(d_qdd), ctypes.c_void_p(stream)))

    def aba_device(self, d_q_qd_tau, N, d_qdd, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_aba_device(self.handle, _ptr(d_q_qd_tau), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N),
                                             ctypes.c_float(gravity), _ptr(d_qdd), ctypes.c_void_p(stream)))

    def idsva_so_device(self, d_q_qd_u, d_qdd, N, d_idsva_so, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_idsva_so_device(self.handle, _ptr(d_q_qd_u), ctypes.c_int(stride or 3 * self.n), _ptr(d_qdd), ctypes.c_int(N),
                                                  ctypes.c_float(gravity), _ptr(d_idsva_so), ctypes.c_void_p(stream)))

    def fdsva_so_device(self, d_q_qd_u, N, d_df2, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_fdsva_so_device(self.handle, _ptr(d_q_qd_u), ctypes.c_int(stride or 3 * self.n), ctypes.c_int(N),
                                                  ctypes.c_float(gravity), _ptr(d_df2), ctypes.c_void_p(stream)))

    def inverse_dynamics_gradient_device(self, d_q_qd, d_qdd, N, d_dc_du, stride=None, gravity=9.81, stream=0):
        self._check(self.lib.grid_inverse_dynamics_gradient_device(self.handle, _ptr(d_q_qd), ctypes.c_int(stride or 3 * self.n), _ptr(d_qdd), ctypes.c_int(N),
                                                                   ctypes.c_float(gravity), _ptr(d_dc_du), ctypes.c_void_p(stream)))


class MultiGpuGrid:
    """One process driving G GPUs: G handles of one robot library, the batch cut into G contiguous ranges.
    `devices` may repeat a device (several handles on one GPU: how the split is rehearsed on a one-GPU box)."""

    def __init__(self, path, devices, max_timesteps=16384):
        self.parts = [GridLibrary(path, device=d, max_timesteps=max_timesteps) for d in devices]
        self.n = self.parts[0].n
        self.lib = self.parts[0].lib

    @staticmethod
    def ranges(N, G):
        """[k0, k1) of every device slot - the same arithmetic as csrc/grid_capi.hip: multi_range."""
        per = (N + G - 1) // G
        return [(min(g * per, N), min((g + 1) * per, N)) for g in range(G)]

    def forward_dynamics_gradient_host(self, q_qd_u, gravity=9.81):
        x = self.parts[0]._host_in(q_qd_u, 3 * self.n, "q_qd_u")
        N = x.shape[0]
        out = np.empty((N, 2 * self.n * self.n), dtype=np.float32)
        hs = (ctypes.c_void_p * len(self.parts))(*[p.handle for p in self.parts])
        rc = self.lib.grid_forward_dynamics_gradient_multi_host(hs, ctypes.c_int(len(self.parts)), _ptr(x), ctypes.c_int(N), ctypes.c_float(gravity), _ptr(out))
        self.parts[0]._check(rc)
        return out

    def close(self):
        for p in self.parts:
            p.close()


def discrete_jacobians(fx, fu, dt):
    """Jacobians of ONE step x_{t+1} = step(x_t, u_t), x = [q; qd], of the semi-implicit Euler integrator of rollout / rollout_linearized, from the
    continuous-time records: fx (..., 2n^2) = [Fq | Fv] stored [col*n + row], fu (..., n^2) = M^-1.  Returns row-major matrices
        A (..., 2n, 2n) = [[I + dt^2 Fq, dt (I + dt Fv)], [dt Fq, I + dt Fv]],   B (..., 2n, n) = [[dt^2 fu], [dt fu]]
    NumPy in -> NumPy out; torch in -> torch out on the same device.  Nothing but this formula: no dynamics is evaluated."""
    n2 = fu.shape[-1]
    n = int(round(n2 ** 0.5))
    if n * n != n2 or fx.shape[-1] != 2 * n2 or tuple(fx.shape[:-1]) != tuple(fu.shape[:-1]):
        raise ValueError("fx must have shape (..., 2n^2) and fu (..., n^2) with the same leading dimensions")
    lead = tuple(fu.shape[:-1])
    if isinstance(fx, np.ndarray):
        F = np.swapaxes(fx.reshape(lead + (2 * n, n)), -1, -2)  # (..., row, col): n x 2n
        M = np.swapaxes(fu.reshape(lead + (n, n)), -1, -2)
        eye = np.eye(n, dtype=fx.dtype)
        cat = np.concatenate
    else:
        import torch

        F = fx.reshape(lead + (2 * n, n)).transpose(-1, -2)
        M = fu.reshape(lead + (n, n)).transpose(-1, -2)
        eye = torch.eye(n, dtype=fx.dtype, device=fx.device)
        cat = lambda parts, axis: torch.cat(parts, dim=axis)
    Fq, Fv = F[..., :n], F[..., n:]
    low_q, low_v = dt * Fq, eye + dt * Fv          # d qd_{t+1} / d q_t, / d qd_t
    top_q, top_v = eye + dt * low_q, dt * low_v    # q_{t+1} = q_t + dt qd_{t+1}
    A = cat([cat([top_q, top_v], -1), cat([low_q, low_v], -1)], -2)
    B = cat([(dt * dt) * M, dt * M], -2)
    return A, B


def gain_records(K):
    """Feedback gains as the closed-loop rollout reads them: row-major matrices K (..., n, 2n) (u = u_ff + K dx) -> records (..., 2n*n) with rec[c*n + j] = K[j, c],
    the [col*n + row] storage of every matrix of the library.  NumPy in -> NumPy out; torch in -> torch out on the same device."""
    if K.ndim < 2 or K.shape[-1] != 2 * K.shape[-2]:
        raise ValueError("K must have shape (..., n, 2n)")
    lead = tuple(K.shape[:-2])
    size = K.shape[-1] * K.shape[-2]
    if isinstance(K, np.ndarray):
        return np.ascontiguousarray(np.swapaxes(K, -1, -2)).reshape(lead + (size,))
    return K.transpose(-1, -2).contiguous().reshape(lead + (size,))


_ROLLOUT_FUNCTION = None


def _rollout_function():
    """The torch.autograd.Function behind GridLibrary.rollout_torch (built on first use: importing this module does not import torch)."""
    global _ROLLOUT_FUNCTION
    if _ROLLOUT_FUNCTION is not None:
        return _ROLLOUT_FUNCTION
    import torch

    def _stream(t):
        return torch.cuda.current_stream(t.device).cuda_stream

    class _RolloutAdjoint(torch.autograd.Function):
        """grad_x0, grad_u = adjoint(traj, u, g): a Function of its own so that a second differentiation meets a backward that says what is missing."""

        @staticmethod
        def forward(ctx, lib, dt, gravity, traj, u, g, want_x0, want_u):
            n, (T1, N) = lib.n, traj.shape[:2]
            T, shared = T1 - 1, u.dim() == 2
            g = g.detach().contiguous()
            gx0 = torch.empty((N, 2 * n), dtype=traj.dtype, device=traj.device) if want_x0 else None
            gu = torch.empty((T, N, n), dtype=traj.dtype, device=traj.device) if (want_u and T > 0) else None
            if gx0 is None and gu is None:
                return None, (torch.zeros_like(u) if want_u else None)
            if traj.is_cuda:
                real, fn = lib._typed("grid_rollout_adjoint_device", traj.dtype == torch.float64)
                with torch.cuda.device(traj.device):
                    lib._rollout_adjoint_device(fn, real, traj, u, N, T, dt, g, None, gx0, gu, shared, gravity, _stream(traj))
            else:
                f = lib.rollout_adjoint_host_f64 if traj.dtype == torch.float64 else lib.rollout_adjoint_host
                res = f(traj.numpy(), u.numpy(), dt, gx=g.numpy(), gravity=gravity, want=tuple(k for k, w in (("grad_x0", gx0 is not None), ("grad_u", gu is not None)) if w))
                for dst, src in zip([o for o in (gx0, gu) if o is not None], res):
                    dst.copy_(torch.from_numpy(src))
            if want_u and gu is None:
                gu = torch.empty((0,) + tuple(u.shape[1:]), dtype=u.dtype, device=u.device)
            elif gu is not None and shared:
                gu = gu.sum(dim=1)
            return gx0, gu

        @staticmethod
        def backward(ctx, *grads):
            raise RuntimeError("rollout_torch is differentiable once: the second-order terms of the rollout (double backward) are not implemented")

    class _Rollout(torch.autograd.Function):
        @staticmethod
        def forward(ctx, lib, dt, gravity, x0, u):
            n = lib.n
            if x0.dtype not in (torch.float32, torch.float64) or u.dtype != x0.dtype or u.device != x0.device:
                raise TypeError("x0 and u must be float32 or float64 tensors of one dtype on one device")
            if x0.dim() != 2 or x0.shape[1] != 2 * n:
                raise ValueError("x0 must have shape (N, 2n) with n = %d" % n)
            N = x0.shape[0]
            x0c = x0.detach().contiguous()
            uc, T, _, _ = lib._u_layout(u.detach().contiguous(), N)
            traj = torch.empty((T + 1, N, 2 * n), dtype=x0.dtype, device=x0.device)
            if x0.is_cuda:
                real, fn = lib._typed("grid_rollout_device", x0.dtype == torch.float64)
                with torch.cuda.device(x0.device):
                    lib._rollout_forward_device(fn, real, x0c, 2 * n, uc, N, T, dt, (traj, None), uc.dim() == 2, gravity, _stream(x0))
            else:
                f = lib.rollout_host_f64 if x0.dtype == torch.float64 else lib.rollout_host
                traj.copy_(torch.from_numpy(f(x0c.numpy(), uc.numpy(), dt, gravity=gravity)))
            ctx.lib, ctx.dt, ctx.gravity = lib, dt, gravity
            ctx.save_for_backward(traj, uc)
            return traj

        @staticmethod
        def backward(ctx, g):
            traj, uc = ctx.saved_tensors
            want_x0, want_u = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
            gx0, gu = _RolloutAdjoint.apply(ctx.lib, ctx.dt, ctx.gravity, traj, uc, g, want_x0, want_u)
            return None, None, None, gx0, gu

    _ROLLOUT_FUNCTION = _Rollout.apply
    return _ROLLOUT_FUNCTION


def load(robot_name, device=0, max_timesteps=16384, build_dir=None):
    return GridLibrary(library_path(robot_name, build_dir), device=device, max_timesteps=max_timesteps)
