// Exercises the generated closed-loop rollout host API as a downstream C++ driver would: init_robotModel / init_grid / init_gridData / rollout_feedback_reserve /
// rollout_feedback<T> / rollout_feedback_single_timing<T> / rollout_feedback_compute_only<T> / close_grid, for T = float and T = double, with torque limits.
// usage: host_api_rollout_feedback_demo <x0.bin (N x 3n doubles)> <u_ff.bin (S x N x n)> <K.bin (S x N x 2n^2)> <xref.bin (S x N x 2n)> <limit> <N> <S> <dt> <out_f32.bin> <out_f64.bin>
// Writes what rollout_feedback left in h_x_traj ((S+1) x N x 2n) and h_uout_traj (S x N x n), one after the other, as doubles, and prints, per precision, the largest
// difference between them and the records of solve 0 left by rollout_feedback_single_timing and the device buffers of rollout_feedback_compute_only read back by hand.
#include "grid.cuh"
#include <vector>

static double worst(double w, double a, double b) {
    double d = a - b;
    d = d < 0 ? -d : d;
    return (d > w || d != d) ? d : w;
}

template <typename T>
static void run(const std::vector<double> &x0, const std::vector<double> &u, const std::vector<double> &K, const std::vector<double> &xref, double limit, int N, int S, double dt,
                const char *out_path) {
    using namespace grid;
    const int n = NUM_JOINTS;
    robotModel<T> *d_robotModel = init_robotModel<T>();
    hipStream_t *streams = init_grid<T>();
    gridData<T> *hd_data = init_gridData<T>(N);
    if (hd_data->d_K_traj != nullptr || hd_data->h_K_traj != nullptr || hd_data->d_xref_traj != nullptr || hd_data->h_xref_traj != nullptr || hd_data->d_uout_traj != nullptr ||
        hd_data->h_uout_traj != nullptr || hd_data->d_u_lim != nullptr || hd_data->h_u_lim != nullptr) {
        fprintf(stderr, "init_gridData must leave the closed-loop rollout buffers null\n");
        exit(3);
    }
    rollout_feedback_reserve<T>(hd_data, N, S);
    for (size_t i = 0; i < x0.size(); i++) hd_data->h_q_qd_u[i] = static_cast<T>(x0[i]);
    for (size_t i = 0; i < u.size(); i++) hd_data->h_u_traj[i] = static_cast<T>(u[i]);
    for (size_t i = 0; i < K.size(); i++) hd_data->h_K_traj[i] = static_cast<T>(K[i]);
    for (size_t i = 0; i < xref.size(); i++) hd_data->h_xref_traj[i] = static_cast<T>(xref[i]);
    for (int j = 0; j < n; j++) { hd_data->h_u_lim[j] = static_cast<T>(-limit); hd_data->h_u_lim[n + j] = static_cast<T>(limit); }
    // ROLLOUT_FB_SUGGESTED_THREADS, or fewer where a block's LDS would exceed the 64 KB a launch may ask for without raising the kernel's limit
    int gpb = ROLLOUT_FB_SUGGESTED_THREADS / GRID_LANES_PER_SOLVE;
    const int fit = static_cast<int>((64 * 1024) / ((ROLLOUT_FB_LDS_PER_SOLVE + ROLLOUT_FB_OUT_PER_SOLVE) * sizeof(T)));
    if (gpb > fit) gpb = fit;
    const int threads = gpb * GRID_LANES_PER_SOLVE;
    dim3 block_dimms((N + gpb - 1) / gpb, 1, 1), thread_dimms(threads, 1, 1);
    const T h = static_cast<T>(dt), g = static_cast<T>(9.81);
    rollout_feedback<T>(hd_data, d_robotModel, h, g, N, S, true, block_dimms, thread_dimms, streams);
    const size_t row = (size_t)N * 2 * n, urow = (size_t)N * n;
    const size_t nx = row * (S + 1), nu = urow * S;
    std::vector<double> out(nx + nu);
    for (size_t i = 0; i < nx; i++) out[i] = static_cast<double>(hd_data->h_x_traj[i]);
    for (size_t i = 0; i < nu; i++) out[nx + i] = static_cast<double>(hd_data->h_uout_traj[i]);
    // compute_only: the inputs are on the device already; zero the output buffers, run, read them back by hand
    std::vector<T> bx(nx), bu(nu);
    gpuErrchk(hipMemcpy(hd_data->d_x_traj, bx.data(), nx * sizeof(T), hipMemcpyHostToDevice));
    gpuErrchk(hipMemcpy(hd_data->d_uout_traj, bu.data(), nu * sizeof(T), hipMemcpyHostToDevice));
    rollout_feedback_compute_only<T>(hd_data, d_robotModel, h, g, N, S, true, block_dimms, thread_dimms);
    gpuErrchk(hipMemcpy(bx.data(), hd_data->d_x_traj, nx * sizeof(T), hipMemcpyDeviceToHost));
    gpuErrchk(hipMemcpy(bu.data(), hd_data->d_uout_traj, nu * sizeof(T), hipMemcpyDeviceToHost));
    double compute_only = 0;
    for (size_t i = 0; i < nx; i++) compute_only = worst(compute_only, out[i], static_cast<double>(bx[i]));
    for (size_t i = 0; i < nu; i++) compute_only = worst(compute_only, out[nx + i], static_cast<double>(bu[i]));
    // solve 0 alone: its controls are rows of n, its gains rows of 2n^2, its references rows of 2n, one per step
    for (int t = 0; t < S; t++) {
        for (int j = 0; j < n; j++) hd_data->h_u_traj[(size_t)t * n + j] = static_cast<T>(u[(size_t)t * urow + j]);
        for (int j = 0; j < 2 * n * n; j++) hd_data->h_K_traj[(size_t)t * 2 * n * n + j] = static_cast<T>(K[(size_t)t * N * 2 * n * n + j]);
        for (int j = 0; j < 2 * n; j++) hd_data->h_xref_traj[(size_t)t * 2 * n + j] = static_cast<T>(xref[(size_t)t * row + j]);
    }
    rollout_feedback_single_timing<T>(hd_data, d_robotModel, h, g, N, S, true, dim3(1, 1, 1), thread_dimms, streams);
    double single = 0;
    for (int t = 0; t <= S; t++) for (int j = 0; j < 2 * n; j++) single = worst(single, out[(size_t)t * row + j], static_cast<double>(hd_data->h_x_traj[(size_t)t * 2 * n + j]));
    for (int t = 0; t < S; t++) for (int j = 0; j < n; j++) single = worst(single, out[nx + (size_t)t * urow + j], static_cast<double>(hd_data->h_uout_traj[(size_t)t * n + j]));
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
    if (argc < 11) { fprintf(stderr, "usage\n"); return 2; }
    const double limit = atof(argv[5]);
    const int N = atoi(argv[6]), S = atoi(argv[7]);
    const double dt = atof(argv[8]);
    const size_t n = grid::NUM_JOINTS;
    std::vector<double> x0((size_t)N * 3 * n), u((size_t)S * N * n), K((size_t)S * N * 2 * n * n), xref((size_t)S * N * 2 * n);
    if (!slurp(argv[1], x0) || !slurp(argv[2], u) || !slurp(argv[3], K) || !slurp(argv[4], xref)) return 2;
    run<float>(x0, u, K, xref, limit, N, S, dt, argv[9]);
    run<double>(x0, u, K, xref, limit, N, S, dt, argv[10]);
    return 0;
}
