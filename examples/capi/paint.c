/*
 * paint.c -- paint a canvas from a stroke image through the C entry of libneube_hip (include/neube_hip.h), without Python: the
 * geometry encoder and the generator behind one handle, feature-blending level 0 (independent tiles), render mode "clear".
 *
 *   paint <R> <f32|h3|f8> <batch> <weights.bin> <encoder.bin> <preproc> <job.bin> <out.bin>
 *
 * The generator has the shipped ("style1") hyper-parameters at output resolution R.  weights.bin holds every generator parameter as
 * fp32, back to back, in nb_generator_param_info order; encoder.bin every encoder parameter likewise, in nb_encoder_param_info order;
 * preproc is an NB_GEOM_PREPROC_* number.  job.bin holds four int32 (H, W, T, crop margin), the padded geometry image [H, W] uint8
 * (255 = background), the tile origins [T, 2] int32 (y, x; also the tiles' noise positions) and the style z [64] fp32.
 *
 * The tiles are cut from the image (nb_geom_tiles_f32), rendered `batch` at a time (nb_generator_forward_geom) and their interiors
 * pasted into the RGBA canvas in tile order (nb_paste_tiles_u8).  Then tile 0 is rendered once more on its own, eagerly and as the
 * replay of a captured hipGraph -- an interactive stroke.  out.bin: the canvas [H, W, 4] uint8, then the stroke's eager and replayed
 * rgba_u8 [R, R, 4].
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
    HIP_OK(hipMalloc(&d, bytes ? bytes : 4));
    if (bytes) HIP_OK(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    return d;
}

typedef int (*info_fn)(int i, char* name, int64_t shape[4], int* ndim, const void* ctx);

/* one device tensor per parameter from a blob of fp32 values in table order (the library copies them; freed by the caller) */
static void** upload_params(const char* path, int count, info_fn info, const void* ctx) {
    size_t bytes = 0;
    const float* blob = (const float*)read_file(path, &bytes);
    void** params = (void**)calloc((size_t)count, sizeof(void*));
    size_t off = 0;
    for (int i = 0; i < count; ++i) {
        char name[128];
        int64_t shape[4];
        int ndim = 0;
        NB_OK_(info(i, name, shape, &ndim, ctx));
        size_t n = 1;
        for (int k = 0; k < ndim; ++k) n *= (size_t)shape[k];
        if ((off + n) * sizeof(float) > bytes) { fprintf(stderr, "%s too short at %s\n", path, name); exit(1); }
        params[i] = to_device(blob + off, n * sizeof(float));
        off += n;
    }
    if (off * sizeof(float) != bytes) { fprintf(stderr, "%s: %zu bytes left over\n", path, bytes - off * sizeof(float)); exit(1); }
    free((void*)blob);
    return params;
}

static int gen_info(int i, char* name, int64_t shape[4], int* ndim, const void* ctx) {
    return nb_generator_param_info((const NbGeneratorConfig*)ctx, i, name, 128, shape, ndim);
}

static int enc_info(int i, char* name, int64_t shape[4], int* ndim, const void* ctx) {
    (void)ctx;
    return nb_encoder_param_info(i, name, 128, shape, ndim);
}

static void free_params(void** params, int count) {
    for (int i = 0; i < count; ++i) HIP_OK(hipFree(params[i]));
    free(params);
}

/* The CSR cell lists of nb_paste_tiles_u8 (include/neube_hip.h, "Cells"): for every NB_CELL_H x NB_CELL_W cell of the canvas, the
 * tiles whose pasted interior [y + crop, y + R - crop) x [x + crop, x + R - crop) touches it, in ascending tile order. */
static void build_cells(const int32_t* yx, int t, int r, int crop, int h, int w, int32_t** off_out, int32_t** list_out, int* ncells_out) {
    const int ncx = (w + NB_CELL_W - 1) / NB_CELL_W, ncy = (h + NB_CELL_H - 1) / NB_CELL_H, ncells = ncx * ncy;
    int32_t* off = (int32_t*)calloc((size_t)ncells + 1, sizeof(int32_t));
    int32_t* fill = (int32_t*)calloc((size_t)ncells, sizeof(int32_t));
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < t; ++i) {
            int y0 = yx[2 * i] + crop, x0 = yx[2 * i + 1] + crop, y1 = yx[2 * i] + r - crop, x1 = yx[2 * i + 1] + r - crop;
            if (y0 < 0) y0 = 0;
            if (x0 < 0) x0 = 0;
            if (y1 > h) y1 = h;
            if (x1 > w) x1 = w;
            if (y1 <= y0 || x1 <= x0) continue;
            for (int cy = y0 / NB_CELL_H; cy <= (y1 - 1) / NB_CELL_H; ++cy)
                for (int cx = x0 / NB_CELL_W; cx <= (x1 - 1) / NB_CELL_W; ++cx) {
                    const int c = cy * ncx + cx;
                    if (pass == 0) off[c + 1]++;
                    else (*list_out)[off[c] + fill[c]++] = i;
                }
        }
        if (pass == 0) {
            for (int c = 0; c < ncells; ++c) off[c + 1] += off[c];
            *list_out = (int32_t*)malloc(sizeof(int32_t) * (size_t)(off[ncells] > 0 ? off[ncells] : 1));
            (*list_out)[0] = 0;
        }
    }
    free(fill);
    *off_out = off;
    *ncells_out = ncells;
}

int main(int argc, char** argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: %s <R> <f32|h3|f8> <batch> <weights.bin> <encoder.bin> <preproc> <job.bin> <out.bin>\n", argv[0]);
        return 1;
    }
    const int R = atoi(argv[1]), batch = atoi(argv[3]), preproc = atoi(argv[6]);
    const int mode = !strcmp(argv[2], "f32") ? NB_CONV_F32 : !strcmp(argv[2], "h3") ? NB_CONV_H3 : !strcmp(argv[2], "f8") ? NB_CONV_F8 : -1;
    if (mode < 0 || batch < 1) { fprintf(stderr, "bad mode or batch\n"); return 1; }

    NbGeneratorConfig cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.z_dim = 64; cfg.w_dim = 64; cfg.img_resolution = R; cfg.mapping_layers = 4; cfg.mapping_lr_multiplier = 0.01f;
    cfg.channel_base = 16384; cfg.channel_max = 128; cfg.conv_clamp = 256.f;
    cfg.num_geom = 2; cfg.geom_channels[0] = 16; cfg.geom_channels[1] = 256;          /* at the default R/8, R/4: the encoder's */
    NB_OK_(nb_generator_encoder_check(&cfg, preproc));

    /* the job */
    size_t jbytes = 0;
    const char* job = (const char*)read_file(argv[7], &jbytes);
    if (jbytes < 16) { fprintf(stderr, "job.bin too short\n"); return 1; }
    int32_t head[4];
    memcpy(head, job, sizeof(head));
    const int H = head[0], W = head[1], T = head[2], crop = head[3];
    const size_t g_bytes = (size_t)H * W, yx_bytes = (size_t)T * 2 * sizeof(int32_t), z_bytes = 64 * sizeof(float);
    if (H < 1 || W < 1 || T < 1 || jbytes != 16 + g_bytes + yx_bytes + z_bytes) { fprintf(stderr, "job.bin: bad size or header\n"); return 1; }
    const int32_t* yx = (const int32_t*)(job + 16 + g_bytes);
    const float* z1 = (const float*)(job + 16 + g_bytes + yx_bytes);

    /* generator + encoder (both copy their parameters) */
    hipStream_t stream;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    const int np = nb_generator_param_count(&cfg), ne = nb_encoder_param_count();
    if (np < 0) { fprintf(stderr, "config: %s\n", nb_last_error()); return 3; }
    const int n_max = batch < T ? batch : T;
    void** gp = upload_params(argv[4], np, gen_info, &cfg);
    NbGenerator* gen = NULL;
    NB_OK_(nb_generator_create(&cfg, (const void* const*)gp, mode, n_max, stream, &gen));
    free_params(gp, np);
    void** ep = upload_params(argv[5], ne, enc_info, NULL);
    NB_OK_(nb_generator_attach_encoder(gen, (const void* const*)ep, preproc, stream));
    free_params(ep, ne);

    /* device inputs: the image, the tile list (noise positions as int64), z repeated over a batch */
    uint8_t* geom_dev = (uint8_t*)to_device(job + 16, g_bytes);
    int32_t* yx_dev = (int32_t*)to_device(yx, yx_bytes);
    int64_t* pos = (int64_t*)malloc(sizeof(int64_t) * 2 * (size_t)T);
    for (int i = 0; i < 2 * T; ++i) pos[i] = yx[i];
    int64_t* pos_dev = (int64_t*)to_device(pos, sizeof(int64_t) * 2 * (size_t)T);
    float* zs = (float*)malloc(z_bytes * (size_t)n_max);
    for (int i = 0; i < n_max; ++i) memcpy(zs + 64 * i, z1, z_bytes);
    float* z_dev = (float*)to_device(zs, z_bytes * (size_t)n_max);
    float* patches = NULL;
    uint8_t *tiles = NULL, *canvas = NULL;
    const size_t tile_bytes = (size_t)R * R * 4;
    HIP_OK(hipMalloc((void**)&patches, (size_t)n_max * R * R * sizeof(float)));
    HIP_OK(hipMalloc((void**)&tiles, tile_bytes * (size_t)T));
    HIP_OK(hipMalloc((void**)&canvas, (size_t)H * W * 4));
    HIP_OK(hipMemsetAsync(canvas, 0, (size_t)H * W * 4, stream));

    NbGeneratorInputs in;
    memset(&in, 0, sizeof(in));
    in.z = z_dev;
    in.truncation_psi = 1.f;
    in.truncation_cutoff = -1;
    in.noise_mode = NB_NOISE_CONST;
    in.render_mode = NB_RENDER_CLEAR;
    NbGeneratorOutputs out;
    memset(&out, 0, sizeof(out));

    /* the canvas: cut, render and paste */
    for (int b0 = 0; b0 < T; b0 += n_max) {
        const int n = T - b0 < n_max ? T - b0 : n_max;
        NB_OK_(nb_geom_tiles_f32(geom_dev, H, W, yx_dev + 2 * b0, n, R, patches, stream));
        in.positions = pos_dev + 2 * b0;
        out.rgba_u8 = tiles + tile_bytes * (size_t)b0;
        NB_OK_(nb_generator_forward_geom(gen, &in, patches, &out, n, stream));
    }
    int32_t *cell_off = NULL, *cell_tiles = NULL;
    int ncells = 0;
    build_cells(yx, T, R, crop, H, W, &cell_off, &cell_tiles, &ncells);
    int32_t* off_dev = (int32_t*)to_device(cell_off, sizeof(int32_t) * ((size_t)ncells + 1));
    int32_t* lst_dev = (int32_t*)to_device(cell_tiles, sizeof(int32_t) * (size_t)(cell_off[ncells] > 0 ? cell_off[ncells] : 1));
    NB_OK_(nb_paste_tiles_u8(tiles, T, R, yx_dev, crop, canvas, H, W, off_dev, lst_dev, stream));
    HIP_OK(hipStreamSynchronize(stream));

    /* one interactive stroke (tile 0, batch 1): eager, then captured into a hipGraph and replayed into another buffer */
    uint8_t* stroke[2] = {NULL, NULL};
    HIP_OK(hipMalloc((void**)&stroke[0], tile_bytes));
    HIP_OK(hipMalloc((void**)&stroke[1], tile_bytes));
    HIP_OK(hipMemsetAsync(stroke[1], 0, tile_bytes, stream));
    NB_OK_(nb_geom_tiles_f32(geom_dev, H, W, yx_dev, 1, R, patches, stream));
    in.positions = pos_dev;
    out.rgba_u8 = stroke[0];
    NB_OK_(nb_generator_forward_geom(gen, &in, patches, &out, 1, stream));      /* (also sets the kernels' attributes at batch 1) */
    HIP_OK(hipStreamSynchronize(stream));
    hipGraph_t graph;
    hipGraphExec_t exec;
    out.rgba_u8 = stroke[1];
    HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    NB_OK_(nb_generator_forward_geom(gen, &in, patches, &out, 1, stream));
    HIP_OK(hipStreamEndCapture(stream, &graph));
    HIP_OK(hipGraphInstantiate(&exec, graph, NULL, NULL, 0));
    HIP_OK(hipGraphLaunch(exec, stream));
    HIP_OK(hipStreamSynchronize(stream));

    /* results */
    const size_t out_bytes = (size_t)H * W * 4 + 2 * tile_bytes;
    uint8_t* host = (uint8_t*)malloc(out_bytes);
    HIP_OK(hipMemcpy(host, canvas, (size_t)H * W * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(host + (size_t)H * W * 4, stroke[0], tile_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(host + (size_t)H * W * 4 + tile_bytes, stroke[1], tile_bytes, hipMemcpyDeviceToHost));
    FILE* fo = fopen(argv[8], "wb");
    if (!fo || fwrite(host, 1, out_bytes, fo) != out_bytes) { perror(argv[8]); return 1; }
    fclose(fo);
    printf("paint: R=%d %s batch %d: %d tiles on a %d x %d canvas, stroke replay %s eager; written to %s\n", R, argv[2], n_max, T, H, W,
           memcmp(host + (size_t)H * W * 4, host + (size_t)H * W * 4 + tile_bytes, tile_bytes) ? "DIFFERS from" : "equals", argv[8]);

    HIP_OK(hipGraphExecDestroy(exec));
    HIP_OK(hipGraphDestroy(graph));
    NB_OK_(nb_generator_destroy(gen));
    void* bufs[] = {geom_dev, yx_dev, pos_dev, z_dev, patches, tiles, canvas, off_dev, lst_dev, stroke[0], stroke[1]};
    for (size_t i = 0; i < sizeof(bufs) / sizeof(bufs[0]); ++i) HIP_OK(hipFree(bufs[i]));
    HIP_OK(hipStreamDestroy(stream));
    free(host); free(pos); free(zs); free(cell_off); free(cell_tiles);
    free((void*)job);
    return 0;
}
