// Host program of tests/test_attention_launcher_args_cpu.py: calls the four forward attention launchers of libsoccdpt_hip.so directly (the path model.cpp and the
// training step take, past the C entries) with one argument wrong each time.  Every call must return non-zero with the expected message BEFORE it touches the
// HIP runtime, so the program runs without a GPU; the tensor pointers are never dereferenced on these paths (a refused call launches nothing).
// Prints one line per call: "<name>\t<return code>\t<message>".
#include <cstdio>
#include <string>

#include "../soccdpt_amd/csrc/kernels.h"

using namespace soccdpt;

int main() {
    static float buf[64];
    const bf16_t* h16 = reinterpret_cast<const bf16_t*>(buf);
    bf16_t* o16 = reinterpret_cast<bf16_t*>(buf);
    const float* f = buf;
    float* fo = buf;
    hipStream_t st = nullptr;
    struct Geo { const char* name; int B, res, ws, shift, heads; };
    const Geo bad[] = {{"shift_negative", 1, 32, 16, -1, 3}, {"shift_ws", 1, 32, 16, 16, 3}, {"shift_not_half", 1, 32, 16, 3, 3}, {"B_zero", 0, 32, 16, 8, 3},
                       {"res_negative", 1, -32, 16, 8, 3}, {"heads_zero", 1, 32, 16, 8, 0}, {"ws_zero", 1, 32, 0, 0, 3}, {"res_mod_ws", 1, 40, 16, 8, 3}};
    for (const Geo& g : bad) {
        std::string err;
        int rc = launch_window_attention(h16, f, f, o16, 1, g.B, g.res, g.ws, g.shift, g.heads, st, err);
        std::printf("window16.%s\t%d\t%s\n", g.name, rc, err.c_str());
        err.clear();
        rc = launch_window_attention_f32(f, f, f, f, fo, g.B, g.res, g.ws, g.shift, g.heads, st, err);
        std::printf("windowf32.%s\t%d\t%s\n", g.name, rc, err.c_str());
        err.clear();
        rc = launch_window_attention_qkv(h16, buf, f, f, f, o16, 1, 0, g.B, g.res, g.ws, g.shift, g.heads, st, err);
        std::printf("qkv.%s\t%d\t%s\n", g.name, rc, err.c_str());
    }
    std::string err;
    int rc = launch_window_attention(nullptr, f, f, o16, 1, 1, 32, 16, 8, 3, st, err);
    std::printf("window16.null_qkv\t%d\t%s\n", rc, err.c_str());
    rc = launch_window_attention(h16, f, f, nullptr, 1, 1, 32, 16, 8, 3, st, err);
    std::printf("window16.null_out\t%d\t%s\n", rc, err.c_str());
    rc = launch_window_attention_f32(f, f, f, nullptr, fo, 1, 32, 16, 8, 3, st, err);
    std::printf("windowf32.null_scale\t%d\t%s\n", rc, err.c_str());
    rc = launch_window_attention_f32(f, nullptr, f, f, fo, 1, 32, 16, 8, 3, st, err);
    std::printf("windowf32.null_bias_acc\t%d\t%s\n", rc, err.c_str());
    rc = launch_window_attention_f32(f, f, nullptr, f, fo, 1, 20, 10, 5, 3, st, err);
    std::printf("windowf32.null_table\t%d\t%s\n", rc, err.c_str());
    rc = launch_window_attention_qkv(h16, nullptr, f, f, f, o16, 1, 0, 1, 32, 16, 8, 3, st, err);
    std::printf("qkv.null_w\t%d\t%s\n", rc, err.c_str());
    rc = launch_attn_bias(nullptr, fo, 16, 3, st, err);
    std::printf("bias.null_table\t%d\t%s\n", rc, err.c_str());
    rc = launch_attn_bias(f, fo, 0, 3, st, err);
    std::printf("bias.ws_zero\t%d\t%s\n", rc, err.c_str());
    rc = launch_vit_attention(nullptr, buf, SOCCDPT_PREC_F16, 1, 33, 12, st, err);
    std::printf("vit.null_qkv\t%d\t%s\n", rc, err.c_str());
    rc = launch_vit_attention(buf, nullptr, SOCCDPT_PREC_F32, 1, 33, 12, st, err);
    std::printf("vit.null_out\t%d\t%s\n", rc, err.c_str());
    rc = launch_vit_attention(buf, buf, SOCCDPT_PREC_BF16, 0, 33, 12, st, err);
    std::printf("vit.B_zero\t%d\t%s\n", rc, err.c_str());
    rc = launch_vit_attention(buf, buf, SOCCDPT_PREC_BF16, 1, 609, 12, st, err);
    std::printf("vit.too_long\t%d\t%s\n", rc, err.c_str());
    rc = launch_vit_attention(buf, buf, SOCCDPT_PREC_BF16, 1, 33, 12, st, err, 1);
    std::printf("vit.x3_not_fp16\t%d\t%s\n", rc, err.c_str());
    return 0;
}
