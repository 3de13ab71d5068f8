// grid_kernel_shell.h - the robot-independent shell of a lane-group kernel: input staging at the head, model constants into registers,
// wave-cooperative copy-out at the tail.  Hand-written device code; the generated header (<namespace>.cuh) includes it and calls it from the
// forward-dynamics-gradient kernel of tip-frame robots with the robot's integers as template arguments.
//
// Execution model it serves: LANES consecutive lanes of ONE wavefront own a solve; the lane groups of a wave own
// consecutive solves, so a wave's records are one contiguous span of global memory and of the LDS staging area behind the block's slices.
// A wave's path through a launch is serial (dispatch -> loads -> compute -> store -> drain): everything here is about leaving ONE exposed
// memory wait at each end of it.
//
// Compiles for gfx950 (hipcc) and as plain C++ in the CPU emulation of the tests (__HIP_DEVICE_COMPILE__ undefined, one host thread per lane).
#ifndef GRID_KERNEL_SHELL_H
#define GRID_KERNEL_SHELL_H

#if defined(__HIP_DEVICE_COMPILE__)
#define GRID_SHELL_FN __device__ __forceinline__
#else
#define GRID_SHELL_FN __device__ inline
#endif

// x, known to be the same on every lane of the wave, as a scalar: the compiler then keeps what is derived from it in SGPRs and branches on it
// with a scalar branch (no exec-mask region)
GRID_SHELL_FN int grid_shell_wave_uniform(const int x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(x);
#else
    return x;
#endif
}

// Pins a value in a register at this point of the program (an empty asm with an in/out operand, as grid_pin of the generated header): the compiler
// neither sinks the load that produces it below this point nor duplicates it.
template <typename T>
GRID_SHELL_FN void grid_shell_pin(T &x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#else
    (void)x;
#endif
}

// Loads N consecutive model constants (a lane's row of grid_model_constants) into registers.  Meant for the head of the kernel, in front of
// grid_shell_load_inputs: the address depends on the lane only, so the loads are in flight together with the input loads and are covered by
// the same wait (vector memory returns in order).  Behind the kernel's first wave-level fence the compiler cannot move them up itself.
template <int N, typename T>
GRID_SHELL_FN void grid_shell_load_constants(T (&c)[N], const T *row) {
    #pragma unroll
    for (int r = 0; r < N; r++) { c[r] = row[r]; }
}

// Stages one solve's input record (IN values at d_in, any 4-byte aligned address: dword loads) in its LDS slice s_in: lane j of the solve's
// lane group moves elements j, j + LANES, ...  Branch-free: an index past the record is clamped to its last element (that lane repeats a
// neighbour's load and store, same value to the same word) instead of masking the load.  All global loads are issued before the first LDS
// write.  Returns the lane's first element (element `lane`: q of the lane's own joint for a [q | qd | u] record), so the caller has it
// without reading LDS back; the other lanes find the record in LDS after the next grid_wave_sync().
template <typename T, int IN, int LANES>
GRID_SHELL_FN T grid_shell_load_inputs(T *s_in, const T *d_in, const int lane) {
    constexpr int TRIPS = (IN + LANES - 1) / LANES;
    T r_in[TRIPS];
    int ind[TRIPS];
    #pragma unroll
    for (int it = 0; it < TRIPS; it++) {
        const int i = lane + it*LANES;
        ind[it] = ((it + 1)*LANES <= IN || i < IN) ? i : IN - 1;
        r_in[it] = d_in[ind[it]];
    }
    #pragma unroll
    for (int it = 0; it < TRIPS; it++) { s_in[ind[it]] = r_in[it]; }
    return r_in[0];
}

// 16-byte store of a finished piece of an output record (the address is only 4-byte aligned in general; gfx950 handles that).
// NT: non-temporal - the record is never re-read by the kernel.
template <bool NT, typename T>
GRID_SHELL_FN void grid_shell_store4(T *dst, const T (&v)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (NT) {
        typedef T vec4_t __attribute__((ext_vector_type(4), aligned(4)));
        vec4_t x = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(x, reinterpret_cast<vec4_t *>(dst));
        return;
    }
#endif
    __builtin_memcpy(dst, v, 4*sizeof(T));
}

// Wave-cooperative copy-out of the records of a wave's lane groups: src is the wave's staging area in LDS (16-byte aligned, the records of
// its SPW lane groups back to back, OUT values each), dst the record of the wave's first solve in global memory.
//   nv: records of this wave that exist (0..SPW; solves past the end of the batch and lane groups past the block's cap do not),
//   wn: lanes of this wave that take part (< 64 in a partial last wave of a block), wl: this lane's index among them.
// nv and wn must be wave-uniform.  A full wave (nv == SPW, wn == 64) takes the straight-line path: every 16-byte LDS read is issued, then
// the stores go out back to back - the trip counts are compile-time constants (7-joint arm: 8 x 98 values = 196 pieces, lanes 0-63 / 64-127 /
// 128-191 / 192-195).  Any other wave takes the general loop: nothing is written at or beyond nv*OUT, the last total % 4 values go out as dwords.
template <typename T, int OUT, int SPW, bool NT>
GRID_SHELL_FN void grid_shell_store_record(T *dst, const T *src, const int nv, const int wn, const int wl) {
    constexpr int TOTAL = SPW*OUT, PIECES = TOTAL/4, TRIPS = (PIECES + 63)/64, TAIL = TOTAL - 4*PIECES;
    constexpr int ALIGN = 4*sizeof(T) < 16 ? 4*sizeof(T) : 16;
    if (nv == SPW && wn == 64) {
        T tmp[TRIPS][4];
        #pragma unroll
        for (int t = 0; t < TRIPS; t++) {
            const int p = wl + 64*t;
            const int pc = ((t + 1)*64 <= PIECES || p < PIECES) ? p : PIECES - 1;  // (the last trip's idle lanes re-read the last piece and store nothing)
            __builtin_memcpy(tmp[t], __builtin_assume_aligned(src + 4*pc, ALIGN), 4*sizeof(T));
        }
        grid_shell_pin(tmp[TRIPS - 1][0]);  // (the last trip's read stays up here with the others instead of sinking into its masked store: one wait for all of them)
        #pragma unroll
        for (int t = 0; t < TRIPS; t++) {
            const int p = wl + 64*t;
            if ((t + 1)*64 <= PIECES || p < PIECES) { grid_shell_store4<NT>(dst + 4*p, tmp[t]); }
        }
        if (TAIL > 0 && wl < TAIL) { dst[4*PIECES + wl] = src[4*PIECES + wl]; }
        return;
    }
    const int total = nv*OUT;  // elements this wave writes
    for (int e = 4*wl; e + 3 < total; e += 4*wn) {
        T tmp[4];
        __builtin_memcpy(tmp, __builtin_assume_aligned(src + e, ALIGN), 4*sizeof(T));
        grid_shell_store4<NT>(dst + e, tmp);
    }
    { const int e = (total & ~3) + wl; if (wl < 3 && e < total) { dst[e] = src[e]; } }
}

#endif  // GRID_KERNEL_SHELL_H
