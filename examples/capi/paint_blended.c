/*
 * paint_blended.c -- paint a SEAMLESS canvas from a stroke image through the C entry of libneube_hip (include/neube_hip.h), without
 * Python: the painting engine's feature blending (levels 1..3; the engine's default is 2), render mode "clear".
 *
 *   paint_blended <R> <f32|h3|f8> <batch> <weights.bin> <encoder.bin> <preproc> <level> <job.bin> <out.bin>
 *
 * Generator, weights.bin, encoder.bin and preproc as in paint.c.  level l blends on the feature canvas at 1 / df of the image
 * resolution, df = 2^(l - 1): the tiles' features behind block R / df.  job.bin is paint.c's job -- four int32 (H, W, T, crop margin),
 * the padded geometry image [H, W] uint8 (255 = background), the tile origins [T, 2] int32 (y, x; also the noise positions), the style
 * z [64] fp32 -- followed by one int32, the blend margin in image pixels (the engine uses 16).
 *
 * Three phases, as painting.PaintingHelper._schedule runs them (the reference walks the tiles one by one, forger/ui/brush.py:190-258):
 *   1  every tile up to the blending block, `batch` at a time (nb_generator_forward_staged, stop_res), into one [T, C, R/df, R/df] buffer
 *   2  one launch blends the tiles on the feature canvas in paint order (nb_canvas_replay_f32), with the alpha template of
 *      nb_dirty_area_alpha_f32 and the cell lists of nb_canvas_build_cells
 *   3  the rest of the generator on the blended features (resume_res), then the paste of the tiles' interiors (nb_paste_tiles_u8)
 * A tile's canvas area is its origin floored to the blending grid (brush.py:253-258).
 *
 * out.bin: the RGBA canvas [H, W, 4] uint8, the feature canvas [C, hc, wc] fp32 and its mask [hc, wc] uint8 (hc = ceil(H / df)).
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

/* the cell lists of `t` rectangles on an h x w grid, on the device (freed by the caller) */
static void cells_to_device(const int32_t* rects, int t, int h, int w, int32_t** off_dev, int32_t** items_dev) {
    const int ncells = ((h + NB_CELL_H - 1) / NB_CELL_H) * ((w + NB_CELL_W - 1) / NB_CELL_W);
    const int count = nb_canvas_cells_count(rects, t, h, w);
    if (count < 0) { fprintf(stderr, "nb_canvas_cells_count: %d %s\n", count, nb_last_error()); exit(3); }
    int32_t* off = (int32_t*)malloc(sizeof(int32_t) * ((size_t)ncells + 1));
    int32_t* items = (int32_t*)malloc(sizeof(int32_t) * (size_t)count);
    if (!off || !items) { fprintf(stderr, "out of memory\n"); exit(1); }
    NB_OK_(nb_canvas_build_cells(rects, t, h, w, off, items));
    *off_dev = (int32_t*)to_device(off, sizeof(int32_t) * ((size_t)ncells + 1));
    *items_dev = (int32_t*)to_device(items, sizeof(int32_t) * (size_t)count);
    free(off);
    free(items);
}

int main(int argc, char** argv) {
    if (argc != 10) {
        fprintf(stderr, "usage: %s <R> <f32|h3|f8> <batch> <weights.bin> <encoder.bin> <preproc> <level> <job.bin> <out.bin>\n", argv[0]);
        return 1;
    }
    const int R = atoi(argv[1]), batch = atoi(argv[3]), preproc = atoi(argv[6]), level = atoi(argv[7]);
    const int mode = !strcmp(argv[2], "f32") ? NB_CONV_F32 : !strcmp(argv[2], "h3") ? NB_CONV_H3 : !strcmp(argv[2], "f8") ? NB_CONV_F8 : -1;
    if (mode < 0 || batch < 1 || level < 1 || level > 3) { fprintf(stderr, "bad mode, batch or level (1..3)\n"); return 1; }

    NbGeneratorConfig cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.z_dim = 64; cfg.w_dim = 64; cfg.img_resolution = R; cfg.mapping_layers = 4; cfg.mapping_lr_multiplier = 0.01f;
    cfg.channel_base = 16384; cfg.channel_max = 128; cfg.conv_clamp = 256.f;
    cfg.num_geom = 2; cfg.geom_channels[0] = 16; cfg.geom_channels[1] = 256;          /* at the default R/8, R/4: the encoder's */
    NB_OK_(nb_generator_encoder_check(&cfg, preproc));
    const int df = 1 << (level - 1), bres = R / df;
    const int C = cfg.channel_base / bres < cfg.channel_max ? cfg.channel_base / bres : cfg.channel_max;     /* channels of block bres */

    /* the job */
    size_t jbytes = 0;
    const char* job = (const char*)read_file(argv[8], &jbytes);
    if (jbytes < 16) { fprintf(stderr, "job.bin too short\n"); return 1; }
    int32_t head[4];
    memcpy(head, job, sizeof(head));
    const int H = head[0], W = head[1], T = head[2], crop = head[3];
    const size_t g_bytes = (size_t)H * W, yx_bytes = (size_t)T * 2 * sizeof(int32_t), z_bytes = 64 * sizeof(float);
    if (H < 1 || W < 1 || T < 1 || crop < 0 || jbytes != 16 + g_bytes + yx_bytes + z_bytes + 4) {
        fprintf(stderr, "job.bin: bad size or header\n");
        return 1;
    }
    const int32_t* yx = (const int32_t*)(job + 16 + g_bytes);
    const float* z1 = (const float*)(job + 16 + g_bytes + yx_bytes);
    int32_t blend_margin = 0;
    memcpy(&blend_margin, job + 16 + g_bytes + yx_bytes + z_bytes, 4);
    const int margin = blend_margin / df, crop_sc = crop / df;            /* on the blending grid */
    const int hc = (H + df - 1) / df, wc = (W + df - 1) / df;

    /* tile areas: origins floored to the blending grid; their rectangles on the feature canvas and their pasted interiors */
    int32_t* floored = (int32_t*)malloc(yx_bytes);
    int32_t* fyx = (int32_t*)malloc(yx_bytes);
    int32_t* frects = (int32_t*)malloc(2 * yx_bytes);
    int32_t* prects = (int32_t*)malloc(2 * yx_bytes);
    for (int i = 0; i < T; ++i) {
        for (int k = 0; k < 2; ++k) {
            if (yx[2 * i + k] < 0) { fprintf(stderr, "job.bin: negative tile origin\n"); return 1; }
            floored[2 * i + k] = yx[2 * i + k] / df * df;
            fyx[2 * i + k] = floored[2 * i + k] / df;
            frects[4 * i + k] = fyx[2 * i + k];
            frects[4 * i + 2 + k] = fyx[2 * i + k] + bres;
            prects[4 * i + k] = floored[2 * i + k] + crop;
            prects[4 * i + 2 + k] = floored[2 * i + k] + R - crop;
        }
    }

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

    /* device inputs and buffers */
    uint8_t* geom_dev = (uint8_t*)to_device(job + 16, g_bytes);
    int32_t* yx_dev = (int32_t*)to_device(yx, yx_bytes);
    int32_t* floored_dev = (int32_t*)to_device(floored, yx_bytes);
    int32_t* fyx_dev = (int32_t*)to_device(fyx, yx_bytes);
    int64_t* pos = (int64_t*)malloc(sizeof(int64_t) * 2 * (size_t)T);
    for (int i = 0; i < 2 * T; ++i) pos[i] = yx[i];
    int64_t* pos_dev = (int64_t*)to_device(pos, sizeof(int64_t) * 2 * (size_t)T);
    float* zs = (float*)malloc(z_bytes * (size_t)n_max);
    for (int i = 0; i < n_max; ++i) memcpy(zs + 64 * i, z1, z_bytes);
    float* z_dev = (float*)to_device(zs, z_bytes * (size_t)n_max);
    const size_t tile_bytes = (size_t)R * R * 4, feat_tile = (size_t)C * bres * bres;
    const size_t fc_bytes = (size_t)C * hc * wc * sizeof(float), mask_bytes = (size_t)hc * wc;
    float *patches = NULL, *feats = NULL, *alpha0 = NULL, *fcanvas = NULL;
    uint8_t *tiles = NULL, *canvas = NULL, *mask_in = NULL, *mask_out = NULL;
    HIP_OK(hipMalloc((void**)&patches, (size_t)n_max * R * R * sizeof(float)));
    HIP_OK(hipMalloc((void**)&feats, feat_tile * sizeof(float) * (size_t)T));
    HIP_OK(hipMalloc((void**)&alpha0, (size_t)bres * bres * sizeof(float)));
    HIP_OK(hipMalloc((void**)&fcanvas, fc_bytes));
    HIP_OK(hipMalloc((void**)&mask_in, mask_bytes));
    HIP_OK(hipMalloc((void**)&mask_out, mask_bytes));
    HIP_OK(hipMalloc((void**)&tiles, tile_bytes * (size_t)T));
    HIP_OK(hipMalloc((void**)&canvas, (size_t)H * W * 4));
    HIP_OK(hipMemsetAsync(fcanvas, 0, fc_bytes, stream));
    HIP_OK(hipMemsetAsync(mask_in, 0, mask_bytes, stream));
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
    NbGeneratorStage stage;
    memset(&stage, 0, sizeof(stage));

    /* phase 1: every tile up to the blending block */
    stage.stop_res = bres;
    for (int b0 = 0; b0 < T; b0 += n_max) {
        const int n = T - b0 < n_max ? T - b0 : n_max;
        NB_OK_(nb_geom_tiles_f32(geom_dev, H, W, yx_dev + 2 * b0, n, R, patches, stream));
        in.positions = pos_dev + 2 * b0;
        stage.features_out = feats + feat_tile * (size_t)b0;
        NB_OK_(nb_generator_forward_staged(gen, &in, patches, &stage, NULL, n, stream));
    }

    /* phase 2: the tiles blended on the feature canvas, in paint order */
    int32_t *foff_dev = NULL, *flst_dev = NULL, *poff_dev = NULL, *plst_dev = NULL;
    NB_OK_(nb_dirty_area_alpha_f32(alpha0, bres, margin, crop_sc, stream));
    cells_to_device(frects, T, hc, wc, &foff_dev, &flst_dev);
    NB_OK_(nb_canvas_replay_f32(feats, T, C, bres, fyx_dev, alpha0, crop_sc, fcanvas, mask_in, mask_out, hc, wc, foff_dev, flst_dev, stream));

    /* phase 3: the rest of the generator on the blended features, then the paste */
    stage.stop_res = 0;
    stage.resume_res = bres;
    stage.features_out = NULL;
    for (int b0 = 0; b0 < T; b0 += n_max) {
        const int n = T - b0 < n_max ? T - b0 : n_max;
        NB_OK_(nb_geom_tiles_f32(geom_dev, H, W, yx_dev + 2 * b0, n, R, patches, stream));      /* (read at level 3 only) */
        in.positions = pos_dev + 2 * b0;
        stage.features_in = feats + feat_tile * (size_t)b0;
        out.rgba_u8 = tiles + tile_bytes * (size_t)b0;
        NB_OK_(nb_generator_forward_staged(gen, &in, patches, &stage, &out, n, stream));
    }
    cells_to_device(prects, T, H, W, &poff_dev, &plst_dev);
    NB_OK_(nb_paste_tiles_u8(tiles, T, R, floored_dev, crop, canvas, H, W, poff_dev, plst_dev, stream));
    HIP_OK(hipStreamSynchronize(stream));

    /* results */
    const size_t out_bytes = (size_t)H * W * 4 + fc_bytes + mask_bytes;
    uint8_t* host = (uint8_t*)malloc(out_bytes);
    if (!host) { fprintf(stderr, "out of memory\n"); return 1; }
    HIP_OK(hipMemcpy(host, canvas, (size_t)H * W * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(host + (size_t)H * W * 4, fcanvas, fc_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(host + (size_t)H * W * 4 + fc_bytes, mask_out, mask_bytes, hipMemcpyDeviceToHost));
    FILE* fo = fopen(argv[9], "wb");
    if (!fo || fwrite(host, 1, out_bytes, fo) != out_bytes) { perror(argv[9]); return 1; }
    fclose(fo);
    printf("paint_blended: R=%d %s batch %d level %d: %d tiles on a %d x %d canvas, %d features blended at %d x %d; written to %s\n", R,
           argv[2], n_max, level, T, H, W, C, hc, wc, argv[9]);

    NB_OK_(nb_generator_destroy(gen));
    void* bufs[] = {geom_dev, yx_dev, floored_dev, fyx_dev, pos_dev, z_dev, patches, feats, alpha0, fcanvas, mask_in, mask_out, tiles, canvas,
                    foff_dev, flst_dev, poff_dev, plst_dev};
    for (size_t i = 0; i < sizeof(bufs) / sizeof(bufs[0]); ++i) HIP_OK(hipFree(bufs[i]));
    HIP_OK(hipStreamDestroy(stream));
    free(host); free(pos); free(zs); free(floored); free(fyx); free(frects); free(prects);
    free((void*)job);
    return 0;
}
