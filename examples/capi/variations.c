/*
 * variations.c -- K variations of one stroke through the C entry of libneube_hip (include/neube_hip.h): the same style and the same
 * geometry, fresh seeded random noise per variation (NB_NOISE_SEEDED, nb_noise_seeded_f32), without Python.
 *
 *   variations <R> <f32|h3|f8> <K> <seed> <offset> <weights.bin> <inputs.bin> <out.bin>
 *
 * The generator has the shipped ("style1") hyper-parameters at output resolution R.  weights.bin is generate.c's; inputs.bin holds
 * z [1, 64] fp32 and the two geometry features [1, 16, R/8, R/8] and [1, 256, R/4, R/4] fp32.  The program makes one eager call,
 * captures the forward into a hipGraph once and replays it K times; before replay i a hipMemcpyAsync writes {seed, offset + i} into
 * the 16 bytes NbGeneratorInputs.noise_state points to, so every replay draws the noise of another sample index.  out.bin: the K
 * tiles rgba_u8 [K, R, R, 4].  Tile i is what a batch of K variations would hold as sample i at (seed, offset).
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
    if (argc != 9) {
        fprintf(stderr, "usage: %s <R> <f32|h3|f8> <K> <seed> <offset> <weights.bin> <inputs.bin> <out.bin>\n", argv[0]);
        return 1;
    }
    const int R = atoi(argv[1]), K = atoi(argv[3]);
    const int mode = !strcmp(argv[2], "f32") ? NB_CONV_F32 : !strcmp(argv[2], "h3") ? NB_CONV_H3 : !strcmp(argv[2], "f8") ? NB_CONV_F8 : -1;
    const uint64_t seed = strtoull(argv[4], NULL, 0), offset = strtoull(argv[5], NULL, 0);
    if (mode < 0 || K < 1) { fprintf(stderr, "bad mode or count\n"); return 1; }

    NbGeneratorConfig cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.z_dim = 64; cfg.w_dim = 64; cfg.img_resolution = R; cfg.mapping_layers = 4; cfg.mapping_lr_multiplier = 0.01f;
    cfg.channel_base = 16384; cfg.channel_max = 128; cfg.conv_clamp = 256.f;
    cfg.num_geom = 2; cfg.geom_channels[0] = 16; cfg.geom_channels[1] = 256;          /* at the default R/8, R/4 */

    /* weights: one device tensor per parameter (the generator copies them; they are freed after creation) */
    const int np = nb_generator_param_count(&cfg);
    if (np < 0) { fprintf(stderr, "config: %s\n", nb_last_error()); return 3; }
    size_t wbytes = 0;
    const float* wblob = (const float*)read_file(argv[6], &wbytes);
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
    NB_OK_(nb_generator_create(&cfg, (const void* const*)params, mode, 1, stream, &gen));
    for (int i = 0; i < np; ++i) HIP_OK(hipFree(params[i]));
    free(params);

    /* one stroke: a style and its geometry; the noise source is a device {seed, offset} pair the graph reads at every replay */
    const size_t z_bytes = 64 * sizeof(float);
    const size_t g0_bytes = (size_t)16 * (R / 8) * (R / 8) * sizeof(float), g1_bytes = (size_t)256 * (R / 4) * (R / 4) * sizeof(float);
    size_t ibytes = 0;
    const char* iblob = (const char*)read_file(argv[7], &ibytes);
    if (ibytes != z_bytes + g0_bytes + g1_bytes) { fprintf(stderr, "inputs.bin: %zu bytes, expected %zu\n", ibytes, z_bytes + g0_bytes + g1_bytes); return 1; }
    uint64_t* states = (uint64_t*)malloc((size_t)K * 2 * sizeof(uint64_t));      /* host copies stay valid until the final synchronisation */
    if (!states) { fprintf(stderr, "out of memory\n"); return 1; }
    for (int i = 0; i < K; ++i) { states[2 * i] = seed; states[2 * i + 1] = offset + (uint64_t)i; }
    uint64_t* state_dev = (uint64_t*)to_device(states, 2 * sizeof(uint64_t));
    NbGeneratorInputs in;
    memset(&in, 0, sizeof(in));
    in.z = (const float*)to_device(iblob, z_bytes);
    in.geom[0] = (const float*)to_device(iblob + z_bytes, g0_bytes);
    in.geom[1] = (const float*)to_device(iblob + z_bytes + g0_bytes, g1_bytes);
    in.truncation_psi = 1.f;
    in.truncation_cutoff = -1;
    in.noise_mode = NB_NOISE_SEEDED;
    in.noise_state = state_dev;
    in.render_mode = NB_RENDER_CLEAR;

    const size_t tile_bytes = (size_t)R * R * 4;
    NbGeneratorOutputs out;
    memset(&out, 0, sizeof(out));
    HIP_OK(hipMalloc((void**)&out.rgba_u8, tile_bytes));
    unsigned char* host = (unsigned char*)malloc((size_t)K * tile_bytes);
    FILE* fo = fopen(argv[8], "wb");
    if (!host || !fo) { perror(argv[8]); return 1; }

    /* one eager call (it also sets the kernels' once-per-process attributes, which a capture must not do), then one capture */
    NB_OK_(nb_generator_forward(gen, &in, &out, 1, stream));
    HIP_OK(hipStreamSynchronize(stream));
    hipGraph_t graph;
    hipGraphExec_t exec;
    HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    NB_OK_(nb_generator_forward(gen, &in, &out, 1, stream));
    HIP_OK(hipStreamEndCapture(stream, &graph));
    HIP_OK(hipGraphInstantiate(&exec, graph, NULL, NULL, 0));

    /* K replays, all enqueued before the one synchronisation: 16 bytes in, one graph launch, one tile out */
    for (int i = 0; i < K; ++i) {
        HIP_OK(hipMemcpyAsync(state_dev, states + 2 * i, 2 * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        HIP_OK(hipGraphLaunch(exec, stream));
        HIP_OK(hipMemcpyAsync(host + (size_t)i * tile_bytes, out.rgba_u8, tile_bytes, hipMemcpyDeviceToHost, stream));
    }
    HIP_OK(hipStreamSynchronize(stream));
    if (fwrite(host, 1, (size_t)K * tile_bytes, fo) != (size_t)K * tile_bytes) { perror(argv[8]); return 1; }
    fclose(fo);
    printf("variations: R=%d %s: %d replays of one graph written to %s\n", R, argv[2], K, argv[8]);

    HIP_OK(hipGraphExecDestroy(exec));
    HIP_OK(hipGraphDestroy(graph));
    NB_OK_(nb_generator_destroy(gen));
    HIP_OK(hipFree(out.rgba_u8));
    HIP_OK(hipFree((void*)in.z));
    HIP_OK(hipFree((void*)in.geom[0]));
    HIP_OK(hipFree((void*)in.geom[1]));
    HIP_OK(hipFree(state_dev));
    HIP_OK(hipStreamDestroy(stream));
    free(host);
    free(states);
    free((void*)wblob);
    free((void*)iblob);
    return 0;
}
