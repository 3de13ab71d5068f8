// Exercises the generated crba host API as a reference-style driver would: init_robotModel / init_grid / init_gridData / crba<T> /
// crba_single_timing<T> / crba_compute_only<T> / close_grid, for T = float and T = double.
// usage: host_api_crba_demo <in.bin (N x 3n doubles)> <N> <out_f32.bin> <out_f64.bin>
// Writes the h_M left by crba (N records of n*n, as doubles) and prints, per precision, the largest difference between it and the h_M left by
// crba_single_timing (3 repetitions: solve 0) and by crba_compute_only (d_M read back by hand).
#include "grid.cuh"
#include <vector>

template <typename T>
static void run(const std::vector<double> &in, int N, const char *out_path) {
    using namespace grid;
    const int nn = NUM_JOINTS * NUM_JOINTS;
    robotModel<T> *d_robotModel = init_robotModel<T>();
    hipStream_t *streams = init_grid<T>();
    gridData<T> *hd_data = init_gridData<T>(N);
    if (hd_data->d_M != nullptr || hd_data->h_M != nullptr) { fprintf(stderr, "init_gridData must leave d_M / h_M null\n"); exit(3); }
    for (size_t i = 0; i < in.size(); i++) hd_data->h_q_qd_u[i] = static_cast<T>(in[i]);
    // CRBA_SUGGESTED_THREADS, or fewer where a block's LDS would exceed the 160 KB of a CU (the humanoid in double precision)
    int gpb = CRBA_SUGGESTED_THREADS / GRID_LANES_PER_SOLVE;
    const int fit = static_cast<int>((160 * 1024) / ((CRBA_LDS_PER_SOLVE + CRBA_OUT_PER_SOLVE) * sizeof(T)));
    if (gpb > fit) gpb = fit;
    const int threads = gpb * GRID_LANES_PER_SOLVE;
    dim3 block_dimms((N + gpb - 1) / gpb, 1, 1), thread_dimms(threads, 1, 1);
    crba<T>(hd_data, d_robotModel, static_cast<T>(9.81), N, block_dimms, thread_dimms, streams);
    std::vector<double> out((size_t)N * nn);
    for (size_t i = 0; i < out.size(); i++) out[i] = static_cast<double>(hd_data->h_M[i]);
    crba_single_timing<T>(hd_data, d_robotModel, static_cast<T>(9.81), 3, dim3(1, 1, 1), thread_dimms, streams);
    double single = 0;
    for (int i = 0; i < nn; i++) { double d = out[i] - static_cast<double>(hd_data->h_M[i]); d = d < 0 ? -d : d; single = d > single ? d : single; }
    std::vector<T> back((size_t)N * nn);
    gpuErrchk(hipMemset(hd_data->d_M, 0, back.size() * sizeof(T)));
    crba_compute_only<T>(hd_data, d_robotModel, static_cast<T>(9.81), N, block_dimms, thread_dimms);
    gpuErrchk(hipMemcpy(back.data(), hd_data->d_M, back.size() * sizeof(T), hipMemcpyDeviceToHost));
    double compute_only = 0;
    for (size_t i = 0; i < back.size(); i++) { double d = out[i] - static_cast<double>(back[i]); d = d < 0 ? -d : d; compute_only = d > compute_only ? d : compute_only; }
    printf("%s: single_timing max|delta| = %.3e\n", sizeof(T) == 4 ? "float" : "double", single);
    printf("%s: compute_only max|delta| = %.3e\n", sizeof(T) == 4 ? "float" : "double", compute_only);
    FILE *f = fopen(out_path, "wb");
    fwrite(out.data(), sizeof(double), out.size(), f);
    fclose(f);
    close_grid<T>(streams, d_robotModel, hd_data);
}

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage\n"); return 2; }
    const int N = atoi(argv[2]);
    std::vector<double> in((size_t)N * 3 * grid::NUM_JOINTS);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(in.data(), sizeof(double), in.size(), f) != in.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    run<float>(in, N, argv[3]);
    run<double>(in, N, argv[4]);
    return 0;
}
