// Host-side execution of the f32-weight products (quant_kernels.hip): the lock-step form over slot groups (gemv_w32_slots_kernel, through the product's
// own dispatch launch_linear_w32 with a.batched) next to the single-utterance kernel it must equal bit for bit, slot after slot (gemv_w32_kernel).
// Built by tests/test_emulated_f32_jobs.py against a patched copy of the kernel source, as sim_driver.cpp is by tests/test_simt_emulation.py.
// Test infrastructure only.
#include "quant_kernels_sim.hip"

#include <cstdarg>
#include <stdexcept>

namespace barkhip {
// what quant_kernels.hip takes from kernels.hip
void kernel_fail(const char * fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    throw std::runtime_error(buf);
}
int crosscheck_mask() { return 0; }
}

using namespace barkhip;

extern "C" {

// B slots through one f32 product.  x [B][K], W [(parity_rows ? 2 : 1) * M][K] f32, bias likewise (may be null), st [B] (step parity selects the rows when
// parity_rows != 0).  epi 3: out [B][ld] = dot (+ bias); epi 1: out [B][M] is the residual row, updated in place.
// route 0: one launch over all slots (a.batched); route 1: gemv_w32_kernel slot after slot.  Returns 0, or -1 when the dispatch refuses the shape.
int sim_w32(int route, const float * W, const float * x, const float * ln_g, const float * ln_b, const float * bias, float * out, const StepState * st,
            int K, int M, int B, int parity_rows, int epi, int ld) {
    LinArgs a;
    a.wq.qs = reinterpret_cast<const uint8_t *>(W); a.wq.qt = QT_F32;
    a.M = M; a.K = K; a.N = 1; a.ln_g = ln_g; a.ln_b = ln_b; a.bias = bias; a.parity_rows = parity_rows;
    a.epi = epi == 1 ? EPI_RESID : EPI_LOGITS; a.ld_out = ld;
    try {
        if (route == 0) {
            a.batched = 1; a.nbatch = B; a.x_f32 = x; a.st = st;
            if (epi == 1) a.res = out; else a.out = out;
            launch_linear_w32(nullptr, a);
        } else {
            for (int b = 0; b < B; b++) {
                a.x_f32 = x + (size_t) b * K; a.st = st + b;
                if (epi == 1) a.res = out + (size_t) b * M; else a.out = out + (size_t) b * ld;
                launch_linear_w32(nullptr, a);
            }
        }
    } catch (const std::exception & e) {
        return -1;
    }
    return 0;
}

int sim_w32_state_size() { return (int) sizeof(StepState); }

}  // extern "C"
