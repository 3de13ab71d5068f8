// Exercises the generated rollout-adjoint host API as a downstream C++ driver would: init_robotModel / init_grid / init_gridData / rollout_adjoint_reserve /
// rollout<T> (which leaves the trajectory in h_x_traj) / rollout_adjoint<T> / rollout_adjoint_single_timing<T> / rollout_adjoint_compute_only<T> / close_grid,
// for T = float and T = double.
// usage: host_api_rollout_adjoint_demo <x0.bin (N x 3n doubles)> <u.bin (S x N x n doubles)> <gx.bin ((S+1) x N x 2n doubles)> <N> <S> <dt> <out_f32.bin> <out_f64.bin>
// Writes what rollout left in h_x_traj ((S+1) x N x 2n) and what rollout_adjoint left in h_gx0 (N x 2n) and h_gu_traj (S x N x n), one after the other, as doubles,
// and prints, per precision, the largest difference between the gradients and the records of solve 0 left by rollout_adjoint_single_timing and the device
// buffers of rollout_adjoint_compute_only read back by hand.
#include "grid.cuh"
#include <vector>

static double worst(double w, double a, double b) {
    double d = a - b;
    d = d < 0 ? -d : d;
    return (d > w || d != d) ? d : w;
}

template <typename T>
static void run(const std::vector<double> &x0, const std::vector<double> &u, const std::vector<double> &gx, int N, int S, double dt, const char *out_path) {
    using namespace grid;
    const int n = NUM_JOINTS;
    robotModel<T> *d_robotModel = init_robotModel<T>();
    hipStream_t *streams = init_grid<T>();
    gridData<T> *hd_data = init_gridData<T>(N);
    if (hd_data->d_gx_traj != nullptr || hd_data->h_gx_traj != nullptr || hd_data->d_gu_traj != nullptr || hd_data->h_gu_traj != nullptr || hd_data->d_gx0 != nullptr ||
        hd_data->h_gx0 != nullptr) {
        fprintf(stderr, "init_gridData must leave the rollout adjoint buffers null\n");
        exit(3);
    }
    rollout_adjoint_reserve<T>(hd_data, N, S);
    for (size_t i = 0; i < x0.size(); i++) hd_data->h_q_qd_u[i] = static_cast<T>(x0[i]);
    for (size_t i = 0; i < u.size(); i++) hd_data->h_u_traj[i] = static_cast<T>(u[i]);
    for (size_t i = 0; i < gx.size(); i++) hd_data->h_gx_traj[i] = static_cast<T>(gx[i]);
    const T h = static_cast<T>(dt), g = static_cast<T>(9.81);
    {  // the forward pass: leaves the trajectory in h_x_traj, where rollout_adjoint reads it
        const int gpb = ROLLOUT_SUGGESTED_THREADS / GRID_LANES_PER_SOLVE;
        rollout<T>(hd_data, d_robotModel, h, g, N, S, dim3((N + gpb - 1) / gpb, 1, 1), dim3(ROLLOUT_SUGGESTED_THREADS, 1, 1), streams);
    }
    // ROLLOUT_ADJ_SUGGESTED_THREADS, or fewer where a block's LDS would exceed the 64 KB a launch may ask for without raising the kernel's limit
    int gpb = ROLLOUT_ADJ_SUGGESTED_THREADS / GRID_LANES_PER_SOLVE;
    const int fit = static_cast<int>((64 * 1024) / ((ROLLOUT_ADJ_LDS_PER_SOLVE + ROLLOUT_ADJ_OUT_PER_SOLVE) * sizeof(T)));
    if (gpb > fit) gpb = fit;
    const int threads = gpb * GRID_LANES_PER_SOLVE;
    dim3 block_dimms((N + gpb - 1) / gpb, 1, 1), thread_dimms(threads, 1, 1);
    rollout_adjoint<T>(hd_data, d_robotModel, h, g, N, S, block_dimms, thread_dimms, streams);
    const size_t row = (size_t)N * 2 * n, gu_row = (size_t)N * n;
    const size_t nx = row * (S + 1), ngu = gu_row * S;
    std::vector<double> out(nx + row + ngu);
    for (size_t i = 0; i < nx; i++) out[i] = static_cast<double>(hd_data->h_x_traj[i]);
    for (size_t i = 0; i < row; i++) out[nx + i] = static_cast<double>(hd_data->h_gx0[i]);
    for (size_t i = 0; i < ngu; i++) out[nx + row + i] = static_cast<double>(hd_data->h_gu_traj[i]);
    // compute_only: the inputs are on the device already; zero the output buffers, run, read them back by hand
    std::vector<T> b0(row), bu(ngu);
    gpuErrchk(hipMemcpy(hd_data->d_gx0, b0.data(), row * sizeof(T), hipMemcpyHostToDevice));
    gpuErrchk(hipMemcpy(hd_data->d_gu_traj, bu.data(), ngu * sizeof(T), hipMemcpyHostToDevice));
    rollout_adjoint_compute_only<T>(hd_data, d_robotModel, h, g, N, S, block_dimms, thread_dimms);
    gpuErrchk(hipMemcpy(b0.data(), hd_data->d_gx0, row * sizeof(T), hipMemcpyDeviceToHost));
    gpuErrchk(hipMemcpy(bu.data(), hd_data->d_gu_traj, ngu * sizeof(T), hipMemcpyDeviceToHost));
    double compute_only = 0;
    for (size_t i = 0; i < row; i++) compute_only = worst(compute_only, out[nx + i], static_cast<double>(b0[i]));
    for (size_t i = 0; i < ngu; i++) compute_only = worst(compute_only, out[nx + row + i], static_cast<double>(bu[i]));
    // solve 0 alone: its states and cotangents are rows of 2n, its controls rows of n, one per step; its records are (2n) and (S, n)
    for (int t = 0; t <= S; t++) for (int j = 0; j < 2 * n; j++) {
        hd_data->h_x_traj[(size_t)t * 2 * n + j] = static_cast<T>(out[(size_t)t * row + j]);
        hd_data->h_gx_traj[(size_t)t * 2 * n + j] = static_cast<T>(gx[(size_t)t * row + j]);
    }
    for (int t = 0; t < S; t++) for (int j = 0; j < n; j++) hd_data->h_u_traj[(size_t)t * n + j] = static_cast<T>(u[((size_t)t * N) * n + j]);
    rollout_adjoint_single_timing<T>(hd_data, d_robotModel, h, g, N, S, dim3(1, 1, 1), thread_dimms, streams);
    double single = 0;
    for (int j = 0; j < 2 * n; j++) single = worst(single, out[nx + j], static_cast<double>(hd_data->h_gx0[j]));
    for (int t = 0; t < S; t++) for (int j = 0; j < n; j++) single = worst(single, out[nx + row + (size_t)t * gu_row + j], static_cast<double>(hd_data->h_gu_traj[(size_t)t * n + j]));
    printf("%s: single_timing max|delta| = %.3e\n", sizeof(T) == 4 ? "float" : "double", single);
    printf("%s: compute_only max|delta| = %.3e\n", sizeof(T) == 4 ? "float" : "double", compute_only);
    FILE *f = fopen(out_path, "wb");
    fwrite(out.data(), sizeof(double), out.size(), f);
    fclose(f);
    close_grid<T>(streams, d_robotModel, hd_data);
}

static bool slurp(const char *path, std::vector<double> &v) {
    FILE *f = fopen(path, "rb");
    const bool ok = f && fread(v.data(), sizeof(double), v.size(), f) == v.size();
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s\n", path);
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 9) { fprintf(stderr, "usage\n"); return 2; }
    const int N = atoi(argv[4]), S = atoi(argv[5]);
    const double dt = atof(argv[6]);
    const size_t n = grid::NUM_JOINTS;
    std::vector<double> x0((size_t)N * 3 * n), u((size_t)S * N * n), gx((size_t)(S + 1) * N * 2 * n);
    if (!slurp(argv[1], x0) || !slurp(argv[2], u) || !slurp(argv[3], gx)) return 2;
    run<float>(x0, u, gx, N, S, dt, argv[7]);
    run<double>(x0, u, gx, N, S, dt, argv[8]);
    return 0;
}
