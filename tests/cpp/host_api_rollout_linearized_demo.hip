// Exercises the generated linearised-rollout host API as a downstream C++ driver would: init_robotModel / init_grid / init_gridData /
// rollout_linearized_reserve / rollout_linearized<T> / rollout_linearized_single_timing<T> / rollout_linearized_compute_only<T> / close_grid,
// for T = float and T = double.
// usage: host_api_rollout_linearized_demo <x0.bin (N x 3n doubles)> <u.bin (S x N x n doubles)> <N> <S> <dt> <out_f32.bin> <out_f64.bin>
// Writes what rollout_linearized left in h_x_traj ((S+1) x N x 2n), h_fx_traj (S x N x 2n^2) and h_fu_traj (S x N x n^2), one after the other, as doubles,
// and prints, per precision, the largest difference between them and the records of solve 0 left by rollout_linearized_single_timing and the device
// buffers of rollout_linearized_compute_only read back by hand.
#include "grid.cuh"
#include <vector>

static double worst(double w, double a, double b) {
    double d = a - b;
    d = d < 0 ? -d : d;
    return (d > w || d != d) ? d : w;
}

template <typename T>
static void run(const std::vector<double> &x0, const std::vector<double> &u, int N, int S, double dt, const char *out_path) {
    using namespace grid;
    const int n = NUM_JOINTS;
    robotModel<T> *d_robotModel = init_robotModel<T>();
    hipStream_t *streams = init_grid<T>();
    gridData<T> *hd_data = init_gridData<T>(N);
    if (hd_data->d_fx_traj != nullptr || hd_data->h_fx_traj != nullptr || hd_data->d_fu_traj != nullptr || hd_data->h_fu_traj != nullptr) {
        fprintf(stderr, "init_gridData must leave the linearised rollout buffers null\n");
        exit(3);
    }
    rollout_linearized_reserve<T>(hd_data, N, S);
    for (size_t i = 0; i < x0.size(); i++) hd_data->h_q_qd_u[i] = static_cast<T>(x0[i]);
    for (size_t i = 0; i < u.size(); i++) hd_data->h_u_traj[i] = static_cast<T>(u[i]);
    // ROLLOUT_LIN_SUGGESTED_THREADS, or fewer where a block's LDS would exceed the 64 KB a launch may ask for without raising the kernel's limit
    int gpb = ROLLOUT_LIN_SUGGESTED_THREADS / GRID_LANES_PER_SOLVE;
    const int fit = static_cast<int>((64 * 1024) / ((ROLLOUT_LIN_LDS_PER_SOLVE + ROLLOUT_LIN_OUT_PER_SOLVE) * sizeof(T)));
    if (gpb > fit) gpb = fit;
    const int threads = gpb * GRID_LANES_PER_SOLVE;
    dim3 block_dimms((N + gpb - 1) / gpb, 1, 1), thread_dimms(threads, 1, 1);
    const T h = static_cast<T>(dt), g = static_cast<T>(9.81);
    rollout_linearized<T>(hd_data, d_robotModel, h, g, N, S, block_dimms, thread_dimms, streams);
    const size_t row = (size_t)N * 2 * n, fx_row = (size_t)N * 2 * n * n, fu_row = (size_t)N * n * n;
    const size_t nx = row * (S + 1), nfx = fx_row * S, nfu = fu_row * S;
    std::vector<double> out(nx + nfx + nfu);
    for (size_t i = 0; i < nx; i++) out[i] = static_cast<double>(hd_data->h_x_traj[i]);
    for (size_t i = 0; i < nfx; i++) out[nx + i] = static_cast<double>(hd_data->h_fx_traj[i]);
    for (size_t i = 0; i < nfu; i++) out[nx + nfx + i] = static_cast<double>(hd_data->h_fu_traj[i]);
    // compute_only: zero the device buffers, run, read them back by hand
    std::vector<T> bx(nx), bfx(nfx), bfu(nfu);
    gpuErrchk(hipMemcpy(hd_data->d_x_traj, bx.data(), nx * sizeof(T), hipMemcpyHostToDevice));
    gpuErrchk(hipMemcpy(hd_data->d_fx_traj, bfx.data(), nfx * sizeof(T), hipMemcpyHostToDevice));
    gpuErrchk(hipMemcpy(hd_data->d_fu_traj, bfu.data(), nfu * sizeof(T), hipMemcpyHostToDevice));
    rollout_linearized_compute_only<T>(hd_data, d_robotModel, h, g, N, S, block_dimms, thread_dimms);
    gpuErrchk(hipMemcpy(bx.data(), hd_data->d_x_traj, nx * sizeof(T), hipMemcpyDeviceToHost));
    gpuErrchk(hipMemcpy(bfx.data(), hd_data->d_fx_traj, nfx * sizeof(T), hipMemcpyDeviceToHost));
    gpuErrchk(hipMemcpy(bfu.data(), hd_data->d_fu_traj, nfu * sizeof(T), hipMemcpyDeviceToHost));
    double compute_only = 0;
    for (size_t i = 0; i < nx; i++) compute_only = worst(compute_only, out[i], static_cast<double>(bx[i]));
    for (size_t i = 0; i < nfx; i++) compute_only = worst(compute_only, out[nx + i], static_cast<double>(bfx[i]));
    for (size_t i = 0; i < nfu; i++) compute_only = worst(compute_only, out[nx + nfx + i], static_cast<double>(bfu[i]));
    // solve 0 alone: its controls are rows of n, one per step; its records are (S+1, 2n), (S, 2n^2), (S, n^2)
    for (int t = 0; t < S; t++) for (int j = 0; j < n; j++) hd_data->h_u_traj[(size_t)t * n + j] = static_cast<T>(u[((size_t)t * N) * n + j]);
    rollout_linearized_single_timing<T>(hd_data, d_robotModel, h, g, N, S, dim3(1, 1, 1), thread_dimms, streams);
    double single = 0;
    for (int t = 0; t <= S; t++) for (int j = 0; j < 2 * n; j++) single = worst(single, out[(size_t)t * row + j], static_cast<double>(hd_data->h_x_traj[(size_t)t * 2 * n + j]));
    for (int t = 0; t < S; t++) for (int j = 0; j < 2 * n * n; j++) single = worst(single, out[nx + (size_t)t * fx_row + j], static_cast<double>(hd_data->h_fx_traj[(size_t)t * 2 * n * n + j]));
    for (int t = 0; t < S; t++) for (int j = 0; j < n * n; j++) single = worst(single, out[nx + nfx + (size_t)t * fu_row + j], static_cast<double>(hd_data->h_fu_traj[(size_t)t * n * n + j]));
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
    if (argc < 8) { fprintf(stderr, "usage\n"); return 2; }
    const int N = atoi(argv[3]), S = atoi(argv[4]);
    const double dt = atof(argv[5]);
    std::vector<double> x0((size_t)N * 3 * grid::NUM_JOINTS), u((size_t)S * N * grid::NUM_JOINTS);
    if (!slurp(argv[1], x0) || !slurp(argv[2], u)) return 2;
    run<float>(x0, u, N, S, dt, argv[6]);
    run<double>(x0, u, N, S, dt, argv[7]);
    return 0;
}
