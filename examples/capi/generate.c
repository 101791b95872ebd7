/*
 * generate.c -- render stroke patches through the C entry of libneube_hip (include/neube_hip.h), without Python.
 *
 *   generate <R> <f32|h3|f8> <n> <weights.bin> <inputs.bin> <out.bin>
 *
 * The generator has the shipped ("style1") hyper-parameters at output resolution R.  weights.bin holds every parameter as fp32,
 * back to back, in nb_generator_param_info order; inputs.bin holds z [n, 64] fp32, the two geometry features [n, 16, R/8, R/8] and
 * [n, 256, R/4, R/4] fp32 and the patch positions [n, 2] int64.  The program does one eager forward, captures a second one into a
 * hipGraph and replays it, and writes for each of the two runs rgba_u8 [n, R, R, 4], uvs [n, 3, R, R] and colors [n, 3, 3] (fp32)
 * to out.bin.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "neube_hip.h"

#define HIP_OK(call)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));  \
            exit(2);                                                                               \
        }                                                                                          \
    } while (0)
#define NB_OK_(call)                                                                               \
    do {                                                                                           \
        int rc_ = (call);                                                                          \
        if (rc_ != NB_OK) {                                                                        \
            fprintf(stderr, "%s:%d: %s: %d %s\n", __FILE__, __LINE__, #call, rc_, nb_last_error()); \
            exit(3);                                                                               \
        }                                                                                          \
    } while (0)

static void* read_file(const char* path, size_t* size) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(1); }
    fseek(f, 0, SEEK_END);
    *size = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    void* buf = malloc(*size ? *size : 1);
    if (!buf || fread(buf, 1, *size, f) != *size) { fprintf(stderr, "%s: read failed\n", path); exit(1); }
    fclose(f);
    return buf;
}

static void* to_device(const void* host, size_t bytes) {
    void* d = NULL;
    HIP_OK(hipMalloc(&d, bytes));
    HIP_OK(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    return d;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: %s <R> <f32|h3|f8> <n> <weights.bin> <inputs.bin> <out.bin>\n", argv[0]);
        return 1;
    }
    const int R = atoi(argv[1]), n = atoi(argv[3]);
    const int mode = !strcmp(argv[2], "f32") ? NB_CONV_F32 : !strcmp(argv[2], "h3") ? NB_CONV_H3 : !strcmp(argv[2], "f8") ? NB_CONV_F8 : -1;
    if (mode < 0 || n < 1) { fprintf(stderr, "bad mode or batch\n"); return 1; }

    NbGeneratorConfig cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.z_dim = 64; cfg.w_dim = 64; cfg.img_resolution = R; cfg.mapping_layers = 4; cfg.mapping_lr_multiplier = 0.01f;
    cfg.channel_base = 16384; cfg.channel_max = 128; cfg.conv_clamp = 256.f;
    cfg.num_geom = 2; cfg.geom_channels[0] = 16; cfg.geom_channels[1] = 256;          /* at the default R/8, R/4 */

    /* weights: one device tensor per parameter (the generator copies them; they are freed after creation) */
    const int np = nb_generator_param_count(&cfg);
    if (np < 0) { fprintf(stderr, "config: %s\n", nb_last_error()); return 3; }
    size_t wbytes = 0;
    const float* wblob = (const float*)read_file(argv[4], &wbytes);
    void** params = (void**)calloc((size_t)np, sizeof(void*));
    size_t off = 0;
    for (int i = 0; i < np; ++i) {
        char name[128];
        int64_t shape[4];
        int ndim = 0;
        NB_OK_(nb_generator_param_info(&cfg, i, name, (int)sizeof(name), shape, &ndim));
        size_t count = 1;
        for (int k = 0; k < ndim; ++k) count *= (size_t)shape[k];
        if ((off + count) * sizeof(float) > wbytes) { fprintf(stderr, "weights.bin too short at %s\n", name); return 1; }
        params[i] = to_device(wblob + off, count * sizeof(float));
        off += count;
    }
    if (off * sizeof(float) != wbytes) { fprintf(stderr, "weights.bin: %zu bytes left over\n", wbytes - off * sizeof(float)); return 1; }

    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    NbGenerator* gen = NULL;
    NB_OK_(nb_generator_create(&cfg, (const void* const*)params, mode, n, stream, &gen));
    for (int i = 0; i < np; ++i) HIP_OK(hipFree(params[i]));
    free(params);

    /* inputs */
    const size_t z_bytes = (size_t)n * 64 * sizeof(float);
    const size_t g0_bytes = (size_t)n * 16 * (R / 8) * (R / 8) * sizeof(float), g1_bytes = (size_t)n * 256 * (R / 4) * (R / 4) * sizeof(float);
    const size_t pos_bytes = (size_t)n * 2 * sizeof(int64_t);
    size_t ibytes = 0;
    const char* iblob = (const char*)read_file(argv[5], &ibytes);
    if (ibytes != z_bytes + g0_bytes + g1_bytes + pos_bytes) { fprintf(stderr, "inputs.bin: %zu bytes, expected %zu\n", ibytes, z_bytes + g0_bytes + g1_bytes + pos_bytes); return 1; }
    NbGeneratorInputs in;
    memset(&in, 0, sizeof(in));
    in.z = (const float*)to_device(iblob, z_bytes);
    in.geom[0] = (const float*)to_device(iblob + z_bytes, g0_bytes);
    in.geom[1] = (const float*)to_device(iblob + z_bytes + g0_bytes, g1_bytes);
    in.positions = (const int64_t*)to_device(iblob + z_bytes + g0_bytes + g1_bytes, pos_bytes);
    in.truncation_psi = 1.f;
    in.truncation_cutoff = -1;
    in.noise_mode = NB_NOISE_CONST;
    in.render_mode = NB_RENDER_CLEAR;

    /* outputs */
    const size_t u8_bytes = (size_t)n * R * R * 4, uvs_bytes = (size_t)n * 3 * R * R * sizeof(float), col_bytes = (size_t)n * 9 * sizeof(float);
    NbGeneratorOutputs out;
    memset(&out, 0, sizeof(out));
    HIP_OK(hipMalloc((void**)&out.rgba_u8, u8_bytes));
    HIP_OK(hipMalloc((void**)&out.uvs, uvs_bytes));
    HIP_OK(hipMalloc((void**)&out.colors, col_bytes));
    unsigned char* host = (unsigned char*)malloc(u8_bytes + uvs_bytes + col_bytes);
    FILE* fo = fopen(argv[6], "wb");
    if (!host || !fo) { perror(argv[6]); return 1; }

    /* 1: eager (also sets the kernels' once-per-process attributes, which a capture must not do) */
    NB_OK_(nb_generator_forward(gen, &in, &out, n, stream));
    HIP_OK(hipStreamSynchronize(stream));
    for (int run = 0; run < 2; ++run) {
        if (run == 1) {
            /* 2: the same forward captured into a graph, outputs cleared, graph replayed */
            hipGraph_t graph;
            hipGraphExec_t exec;
            HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            NB_OK_(nb_generator_forward(gen, &in, &out, n, stream));
            HIP_OK(hipStreamEndCapture(stream, &graph));
            HIP_OK(hipGraphInstantiate(&exec, graph, NULL, NULL, 0));
            HIP_OK(hipMemsetAsync(out.rgba_u8, 0, u8_bytes, stream));
            HIP_OK(hipMemsetAsync(out.uvs, 0, uvs_bytes, stream));
            HIP_OK(hipMemsetAsync(out.colors, 0, col_bytes, stream));
            HIP_OK(hipGraphLaunch(exec, stream));
            HIP_OK(hipStreamSynchronize(stream));
            HIP_OK(hipGraphExecDestroy(exec));
            HIP_OK(hipGraphDestroy(graph));
        }
        HIP_OK(hipMemcpy(host, out.rgba_u8, u8_bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(host + u8_bytes, out.uvs, uvs_bytes, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(host + u8_bytes + uvs_bytes, out.colors, col_bytes, hipMemcpyDeviceToHost));
        if (fwrite(host, 1, u8_bytes + uvs_bytes + col_bytes, fo) != u8_bytes + uvs_bytes + col_bytes) { perror(argv[6]); return 1; }
    }
    fclose(fo);
    printf("generate: R=%d %s n=%d: eager + graph replay written to %s\n", R, argv[2], n, argv[6]);

    NB_OK_(nb_generator_destroy(gen));
    HIP_OK(hipFree(out.rgba_u8));
    HIP_OK(hipFree(out.uvs));
    HIP_OK(hipFree(out.colors));
    HIP_OK(hipFree((void*)in.z));
    HIP_OK(hipFree((void*)in.geom[0]));
    HIP_OK(hipFree((void*)in.geom[1]));
    HIP_OK(hipFree((void*)in.positions));
    HIP_OK(hipStreamDestroy(stream));
    free(host);
    free((void*)wblob);
    free((void*)iblob);
    return 0;
}
