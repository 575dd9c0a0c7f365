// svo_kernels_prior.hip — k_prior_predict: the predicted motion prior of SVO_PRIOR_LAST_ROTATION (include/svo.h, "Motion prior").
// The first launch of a frame on the frame's stream: it turns each launched sequence's last pose (SeqState::R, written by the previous
// frame's k_pnp_final on the same stream) into the PriorRow that k_lk_chain_prior reads, before anything of this frame runs the
// per-frame reset that clears SeqState::ok.  A translation unit of its own, like svo_kernels_lk_prior.hip: the code objects of the
// three kernel files hold what they always held.
#include "svo_internal.hpp"
#include "svo_prior.hpp"

// One thread per launched sequence.  act: the n sequence numbers that take the frame, or null: sequence b is thread b.  It is the
// frame's own copy in mapped host memory, not DevBuffers::act: a many-sequence frame uploads that one on its image stream, which is
// not ordered before this launch.  rows / host_rows: the frame's device row and its row of the pinned ring ([B], indexed by sequence).
// uploaded: the host copied its rows into `rows` in front of this launch (some sequence has an explicit prior); 0: `rows` is stale and
// every launched sequence's row is written.  A written row goes to both places: the device row feeds k_lk_chain_prior, the pinned
// one is what svo_get_last_motion_prior reports after the frame's collect (an explicit row is there already, the host wrote it).
__global__ __launch_bounds__(64) void k_prior_predict(const SeqState* __restrict__ st, const int* __restrict__ act, int n, int uploaded, PriorRow* __restrict__ rows,
                                PriorRow* __restrict__ host_rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int seq = act ? act[b] : b;
    const SeqState& s = st[seq];
    PriorRow row = rows[seq];
    double R[9]; float Pl[12];
    for (int k = 0; k < 9; k++) R[k] = s.R[k];
    for (int k = 0; k < 12; k++) Pl[k] = s.Pl[k];
    if (!prior_predict_row(&row, uploaded != 0, s.ok, s.frame_id, R, Pl)) return;
    rows[seq] = row;
    host_rows[seq] = row;
}

void launch_prior_predict(const DevBuffers& d, const int* act, int n, bool uploaded, PriorRow* rows, PriorRow* host_rows, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_prior_predict, dim3((n + 63) / 64), dim3(64), 0, st, d.st, act, n, uploaded ? 1 : 0, rows, host_rows);
}
