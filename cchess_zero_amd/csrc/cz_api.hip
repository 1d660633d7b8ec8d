// cz_api.hip — what libcchess_hip.so has that belongs to no kernel: the error state, cz_crc32c, cz_version, the table getters,
// cz_create / cz_destroy, the stream, synchronize, malloc / free / upload / download, and cz_set_batch_count.  Every other entry
// point of include/cchess_hip.h is defined in the file that holds its kernels.
#include "cz_internal.h"
#include "cz_maskgen.h"

#include <stdarg.h>
#include <string.h>

static thread_local char g_err[512] = "";

void cz_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

void carve_pool(Carver &c, CzPool &p, size_t n) {
    p.P = c.take<float>(n); p.W = c.take<float>(n); p.Q = c.take<float>(n);
    p.N = c.take<int32_t>(n); p.parent = c.take<int32_t>(n); p.child_begin = c.take<int32_t>(n);
    p.child_count = c.take<uint16_t>(n); p.move = c.take<uint16_t>(n); p.sd = c.take<uint16_t>(n);
}

void carve_trees(Carver &c, CzTrees &t, size_t G, size_t words) {
    t.mark_bits = c.take<unsigned long long>(G * words);
    t.mark_rank = c.take<uint32_t>(G * words);
    t.root_board = c.take<uint8_t>(G * CZD_BOARD_LDS);
    t.rec = c.take<CzTreeRec>(G);
    t.pend_moves = c.take<uint16_t>(G * CZD_MAXMOVES);
    t.pend_path = c.take<int32_t>(G * CZ_PATH_MAX);
    t.pk_kind = c.take<int32_t>(G); t.pk_leaf = c.take<int32_t>(G); t.pk_value = c.take<float>(G);
    t.pk_side = c.take<uint8_t>(G); t.pk_nmoves = c.take<uint16_t>(G);
    t.slot_of = c.take<int32_t>(G);
    t.evcnt = c.take<int32_t>(2);
    t.adv_list = c.take<int32_t>(G); t.adv_cnt = c.take<int32_t>(4);
    t.evtotal = c.take<unsigned long long>(2);
}

}  // namespace

extern "C" {

const char *cz_last_error(void) { return g_err; }

// CRC-32C (Castagnoli, reflected 0x82F63B78), host code: the checksum of TensorFlow's checkpoint blocks and tensors
// (cchess_zero_amd/tf_checkpoint.py reads and writes the reference's tf.train.Saver files; pure Python does ~5 MB/s)
unsigned int cz_crc32c(const void *data, size_t n) {
    static unsigned int T[8][256];
    static bool init = false;
    if (!init) {
        for (unsigned int i = 0; i < 256; ++i) {
            unsigned int c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            T[0][i] = c;
        }
        for (unsigned int i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) T[s][i] = (T[s - 1][i] >> 8) ^ T[0][T[s - 1][i] & 0xFFu];
        init = true;
    }
    const unsigned char *p = (const unsigned char *)data;
    unsigned int c = 0xFFFFFFFFu;
    while (n >= 8) {   // slicing-by-8
        const unsigned int lo = c ^ ((unsigned int)p[0] | ((unsigned int)p[1] << 8) | ((unsigned int)p[2] << 16) | ((unsigned int)p[3] << 24));
        c = T[7][lo & 0xFFu] ^ T[6][(lo >> 8) & 0xFFu] ^ T[5][(lo >> 16) & 0xFFu] ^ T[4][lo >> 24] ^
            T[3][p[4]] ^ T[2][p[5]] ^ T[1][p[6]] ^ T[0][p[7]];
        p += 8; n -= 8;
    }
    while (n--) c = T[0][(c ^ *p++) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
int cz_version(void) { return 200; }

int cz_tables(const int16_t **lut, const int16_t **unflip, const char **labels, const uint16_t **srcdst) {
    const CzHostTables &t = cz_host_tables();
    if (lut) *lut = t.lut;
    if (unflip) *unflip = t.unflip;
    if (labels) *labels = t.labels;
    if (srcdst) *srcdst = t.srcdst;
    return CZ_OK;
}

int cz_mirror_table(const int16_t **mirror) {
    if (mirror) *mirror = cz_host_tables().mirror;
    return CZ_OK;
}

int cz_zobrist(const uint64_t **keys, uint64_t *side_key) {
    const CzHostTables &t = cz_host_tables();
    if (keys) *keys = t.zob;
    if (side_key) *side_key = t.zob[15 * CZ_NSQ];
    return CZ_OK;
}

// cz_create's device side: the tables, the per-tree arrays, the node pools.  Whatever fails, the context stays destroyable.
static int create_device_state(cz_ctx *c) {
    const CzHostTables &ht = cz_host_tables();
    int16_t *lut = nullptr, *unf = nullptr, *mir = nullptr;
    uint16_t *sd = nullptr;
    uint64_t *zb = nullptr;
    if (const int rc = carve_alloc(&c->tab_block, c->stream, false, "cz_create (tables)", [&](Carver &k) {
            lut = k.take<int16_t>(CZ_NSQ * CZ_NSQ);
            unf = k.take<int16_t>(CZ_NLABELS);
            sd = k.take<uint16_t>(CZ_NLABELS);
            zb = k.take<uint64_t>(15 * CZ_NSQ + 1);
            mir = k.take<int16_t>(CZ_NLABELS);
        }))
        return rc;
    CZ_HIP(hipMemcpy(lut, ht.lut, sizeof(ht.lut), hipMemcpyHostToDevice));
    CZ_HIP(hipMemcpy(unf, ht.unflip, sizeof(ht.unflip), hipMemcpyHostToDevice));
    CZ_HIP(hipMemcpy(sd, ht.srcdst, sizeof(ht.srcdst), hipMemcpyHostToDevice));
    CZ_HIP(hipMemcpy(zb, ht.zob, sizeof(ht.zob), hipMemcpyHostToDevice));
    CZ_HIP(hipMemcpy(mir, ht.mirror, sizeof(ht.mirror), hipMemcpyHostToDevice));
    c->tab.lut = lut; c->tab.unflip = unf; c->tab.srcdst = sd; c->tab.zob = zb;
    c->tab_mirror = mir;
    CzmTables mt = {};   // the mask-only generator's per-square tables, derived from the label LUT
    czm_build_tables(ht.lut, &mt);
    CzmTables *dmt = nullptr;
    if (hipMalloc(&dmt, sizeof(CzmTables)) != hipSuccess) { cz_set_error("cz_create: hipMalloc(mask tables) failed"); return CZ_ENOMEM; }
    c->mask_tab = dmt;
    CZ_HIP(hipMemcpy(dmt, &mt, sizeof(mt), hipMemcpyHostToDevice));
    // per-tree arrays, zeroed
    const size_t G = (size_t)c->max_games, words = ((size_t)c->cap + 63) / 64;
    if (const int rc = carve_alloc(&c->tree_block, c->stream, true, "cz_create (trees)", [&](Carver &k) { carve_trees(k, c->t, G, words); })) return rc;
    c->t.cap = c->cap;
    c->t.words = (int)words;
    // node pool: ONE pool of cap nodes per tree (cz_search_advance compacts the kept subtree in place)
    if (const int rc = carve_alloc(&c->pool_block, c->stream, false, "cz_create (node pool)", [&](Carver &k) { carve_pool(k, c->t.pool, G * (size_t)c->cap); }))
        return rc;
    CZ_HIP(hipStreamSynchronize(c->stream));   // the zeros stand before the caller binds another stream
    return CZ_OK;
}

int cz_create(int device, int max_games, int max_nodes_per_tree, cz_ctx **out) {
    CZ_REQUIRE(out != nullptr, "cz_create: out is NULL");
    CZ_REQUIRE(max_games > 0 && max_nodes_per_tree >= 2, "cz_create: max_games > 0 and max_nodes_per_tree >= 2 required");
    int ndev = 0;
    CZ_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { cz_set_error("cz_create: device %d not available (%d HIP devices)", device, ndev); return CZ_EINVAL; }
    CZ_HIP(hipSetDevice(device));
    cz_ctx *c = new cz_ctx();
    memset(c, 0, sizeof(*c));
    c->device = device; c->stream = nullptr; c->max_games = max_games; c->cap = max_nodes_per_tree; c->G = 0;
    c->width = 1;
    if (const int rc = create_device_state(c)) {   // cz_destroy frees what a half-built context holds: the struct was zeroed
        cz_destroy(c);
        return rc;
    }
    *out = c;
    return CZ_OK;
}

void cz_destroy(cz_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->pend_block) (void)hipFree(c->pend_block);
    if (c->tab_block) (void)hipFree(c->tab_block);
    if (c->mask_tab) (void)hipFree(const_cast<CzmTables *>(c->mask_tab));
    if (c->xc_block) (void)hipFree(c->xc_block);
    if (c->tree_block) (void)hipFree(c->tree_block);
    if (c->pool_block) (void)hipFree(c->pool_block);
    if (c->sp_block) (void)hipFree(c->sp_block);
    if (c->sp_resign_block) (void)hipFree(c->sp_resign_block);
    cz_root_free(c->sp_root);
    if (c->ec_block) (void)hipFree(c->ec_block);
    delete c;
}

int cz_set_stream(cz_ctx *c, void *s) {
    CZ_REQUIRE(c, "null ctx");
    c->stream = (hipStream_t)s;
    return CZ_OK;
}

int cz_synchronize(cz_ctx *c) {
    CZ_REQUIRE(c, "null ctx");
    CZ_HIP(hipStreamSynchronize(c->stream));
    return CZ_OK;
}

int cz_malloc(cz_ctx *c, size_t bytes, void **dptr) {
    CZ_REQUIRE(c && dptr, "cz_malloc: null argument");
    CZ_HIP(hipSetDevice(c->device));
    if (hipMalloc(dptr, bytes ? bytes : 1) != hipSuccess) { cz_set_error("cz_malloc: %zu bytes failed", bytes); return CZ_ENOMEM; }
    return CZ_OK;
}
int cz_free(cz_ctx *c, void *dptr) {
    CZ_REQUIRE(c, "null ctx");
    CZ_HIP(hipFree(dptr));
    return CZ_OK;
}
int cz_upload(cz_ctx *c, void *dst, const void *src, size_t bytes) {
    CZ_REQUIRE(c, "null ctx");
    CZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    CZ_HIP(hipStreamSynchronize(c->stream));
    return CZ_OK;
}
int cz_download(cz_ctx *c, void *dst, const void *src, size_t bytes) {
    CZ_REQUIRE(c, "null ctx");
    CZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    CZ_HIP(hipStreamSynchronize(c->stream));
    return CZ_OK;
}

int cz_set_batch_count(cz_ctx *c, const int32_t *n_rows_dev) {
    CZ_REQUIRE(c, "null ctx");
    c->batch_count = n_rows_dev;
    return CZ_OK;
}

}  // extern "C"
