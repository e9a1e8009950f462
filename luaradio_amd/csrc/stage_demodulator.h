// stage_demodulator.h - PulseAmplitudeDemodulatorBlock and QuadratureAmplitudeDemodulatorBlock (kernels_demodulator.h), created through lrhip_unary_create
// ("pamdemod:period=P:offset=o:bits=b:msb=0|1:soft=0|1:weight=w:grid=1:table=a0,a1,..." and "qamdemod:...:grid=qb|-1:table=re0,im0,re1,im1,...").
// The only state is the absolute input position: symbol s is emitted by the call that delivers sample s P + offset, so the output count follows from the
// lengths alone and run() reads nothing back.
// (part of liblrhip.so; included by lrhip.hip after stage_modulator.h, one translation unit)
#pragma once

struct DemodStage : lrhip_stage {
    unsigned P = 1, offset = 0;
    int b = 1, msb = 1, ni = 0, nq = 0, ibits = 0, qbits = 0;
    bool qam = false, soft = false, general = false;
    float w = 1.0f;
    DeviceBuf d_table;                       // general: 2^b re, im pairs; grid: the I axis then the Q axis; each padded with NaN to a multiple of DEM_BLOCK entries
    unsigned long long pos = 0;              // input samples consumed so far
    const char *kind() const override { return qam ? "qamdemod" : "pamdemod"; }
    int reset() override { pos = 0; return 0; }
    // symbols whose sample lies below stream position n: ceil((n - offset) / P), 0 while n <= offset
    unsigned long long symbols_before(unsigned long long n) const { return n <= offset ? 0 : (n - offset + P - 1) / P; }
    unsigned long max_output(unsigned long n) const override { return (n / P + 1) * (unsigned long)b; }
    void rate(unsigned long *num, unsigned long *den) const override { *num = P; *den = (unsigned long)b; }
    int seek(unsigned long long n0, unsigned long long *n0_out) override
    {
        pos = n0;
        *n0_out = symbols_before(n0) * (unsigned long long)b;
        return 0;
    }
    template <typename T, int PER>
    int launch(const T *x, const DemodParams &p, void *out_dev)
    {
        const int npi = (ni + DEM_BLOCK - 1) / DEM_BLOCK * DEM_BLOCK, npq = (nq + DEM_BLOCK - 1) / DEM_BLOCK * DEM_BLOCK;
        const int stage_i = general || ni <= (1 << DEM_LDS_AXIS_BITS), stage_q = !general && nq && nq <= (1 << DEM_LDS_AXIS_BITS);
        const size_t lds_bytes = general ? (size_t)npi * sizeof(float2) : ((stage_i ? npi : 0) + (stage_q ? npq : 0)) * sizeof(float);
        const int packed = !soft && (b == 2 || b == 4 || b == 8 || b == 16) && (uintptr_t)out_dev % (uintptr_t)b == 0;
        const long ntiles = (long)((p.nsym + (unsigned long)DEM_NT * PER - 1) / ((unsigned long)DEM_NT * PER));
        auto go = [&](auto kern) -> int {
            const long slots = chip_slots(kern, DEM_NT, lds_bytes);
            if (slots < 0) return -1;
            const unsigned grid = persistent_grid(ntiles, slots, 0);           // a workgroup stages the table once and strides through the tiles
            hipLaunchKernelGGL(kern, dim3(grid ? grid : 1), dim3(DEM_NT), lds_bytes, ctx().stream, x, (const float *)d_table.p, out_dev, p, stage_i, stage_q, packed,
                               (unsigned long)ntiles);
            return 0;
        };
        int rc;
        if constexpr (sizeof(T) == 8) {
            if (general) rc = soft ? go(demod_kernel<T, true, true, PER>) : go(demod_kernel<T, true, false, PER>);
            else rc = soft ? go(demod_kernel<T, false, true, PER>) : go(demod_kernel<T, false, false, PER>);
        } else {
            rc = soft ? go(demod_kernel<T, false, true, PER>) : go(demod_kernel<T, false, false, PER>);
        }
        if (rc) return rc;
        LR_LAUNCH_CHECK();
        return 0;
    }
    long run(const void *in_dev, unsigned long n, void *out_dev, unsigned long cap) override
    {
        if (!n) return 0;
        if (pos + n < pos) return set_error("%s: more than 2^64 input samples", kind());
        const unsigned long long s0 = symbols_before(pos), s1 = symbols_before(pos + n);
        const unsigned long nsym = (unsigned long)(s1 - s0), n_out = nsym * (unsigned long)b;
        if (n_out > cap) return set_error("%s: output capacity %lu < %lu", kind(), cap, n_out);
        if (nsym) {
            if (!in_dev) return set_error("%s: null input buffer", kind());
            if (!out_dev) return set_error("%s: null output buffer", kind());
            // (the first symbol's sample s0 P + offset is at or behind pos, the last one below pos + n)
            const DemodParams p{P, b, msb, ni, nq, ibits, qbits, w, (unsigned long)(s0 * P + offset - pos), nsym};
            int rc;
            if (qam) {
                const float2 *x = (const float2 *)in_dev;
                rc = P == 1 && (uintptr_t)(x + p.first) % 16 == 0 ? launch<float2, 2>(x, p, out_dev) : launch<float2, 1>(x, p, out_dev);
            } else {
                const float *x = (const float *)in_dev;
                rc = P == 1 && (uintptr_t)(x + p.first) % 16 == 0 ? launch<float, 4>(x, p, out_dev) : launch<float, 1>(x, p, out_dev);
            }
            if (rc) return rc;
        }
        pos += n;
        return (long)n_out;
    }
};

// "qamdemod:period=P:offset=o:bits=b:msb=0|1:soft=0|1:weight=w:grid=qb|-1:table=re0,im0,...": the table as the modulators' (%.9g or hexadecimal
// floating-point text), already scaled to the received constellation.  grid=qb: table[v] = (I[v >> qb], Q[v & (2^qb - 1)]) bit for bit, which is checked
// here, and the decision is made per axis; grid=-1: the general search, b <= 12.  "pamdemod" has one axis and takes grid=1 alone.
static lrhip_stage_t *demodulator_create(const char *op)
{
    OpFields f;
    long P = 0, offset = 0, b = 0, msb = 0, soft = 0, grid = 0;
    double weight = 0.0;
    std::vector<float> table;
    if (!f.split(op, nullptr, {{"period", nullptr}, {"offset", nullptr}, {"bits", nullptr}, {"msb", nullptr}, {"soft", nullptr}, {"weight", nullptr},
                               {"grid", nullptr}, {"table", nullptr}}, false) ||
        !f.integer("period", LONG_MIN, LONG_MAX, P) || !f.integer("offset", LONG_MIN, LONG_MAX, offset) || !f.integer("bits", LONG_MIN, LONG_MAX, b) ||
        !f.integer("msb", LONG_MIN, LONG_MAX, msb) || !f.integer("soft", LONG_MIN, LONG_MAX, soft) || !f.number("weight", weight) ||
        !f.integer("grid", LONG_MIN, LONG_MAX, grid) || !f.floats("table", table, 0, "table entry", "", "the table ends")) return nullptr;
    const std::string &name = f.name;
    const bool qam = name == "qamdemod";
    if (P < 1 || P >= (1l << 30)) { set_error("%s: period must be 1 .. 2^30 - 1 samples per symbol (got %ld)", name.c_str(), P); return nullptr; }
    if (offset < 0 || offset >= P) { set_error("%s: offset must be 0 .. period - 1 = %ld (got %ld)", name.c_str(), P - 1, offset); return nullptr; }
    if (b < 1 || b > MOD_MAX_BITS) { set_error("%s: bits per symbol must be 1 .. %d (got %ld)", name.c_str(), MOD_MAX_BITS, b); return nullptr; }
    if (msb != 0 && msb != 1) { set_error("%s: msb must be 0 or 1", name.c_str()); return nullptr; }
    if (soft != 0 && soft != 1) { set_error("%s: soft must be 0 or 1", name.c_str()); return nullptr; }
    const float w = (float)weight;
    if (!(w > 0.0f) || !std::isfinite(w)) { set_error("%s: weight must be a finite Float32 above 0 (got %g)", name.c_str(), weight); return nullptr; }
    if (!qam && grid != 1) { set_error("%s: grid must be 1, the one axis (got %ld)", name.c_str(), grid); return nullptr; }
    if (qam && (grid < -1 || grid > b)) { set_error("%s: grid must be -1 (general search) or the 0 .. %ld low bits of the second axis (got %ld)", name.c_str(), b, grid); return nullptr; }
    const bool general = qam && grid < 0;
    if (general && b > DEM_GENERAL_MAX_BITS) {
        set_error("%s: a table that is no grid is limited to %d bits per symbol, 2^%d entries (got %ld)", name.c_str(), DEM_GENERAL_MAX_BITS, DEM_GENERAL_MAX_BITS, b);
        return nullptr;
    }
    const size_t count = (size_t)1 << b, want = count * (qam ? 2 : 1);
    if (table.size() != want) { set_error("%s: the table has %zu values, %d bits per symbol need %zu", name.c_str(), table.size(), (int)b, want); return nullptr; }
    // the image the kernels read, each part padded with NaN to whole blocks of the soft search
    const int qbits = qam && !general ? (int)grid : 0, ibits = (int)b - qbits;
    const size_t ni = general ? count : (size_t)1 << ibits, nq = qam && !general ? (size_t)1 << qbits : 0;
    auto padded = [](size_t n) { return (n + DEM_BLOCK - 1) / DEM_BLOCK * DEM_BLOCK; };
    std::vector<float> image;
    if (general) {
        image.assign(2 * padded(count), NAN);
        std::copy(table.begin(), table.end(), image.begin());
    } else {
        image.assign(padded(ni) + padded(nq), NAN);
        for (size_t i = 0; i < ni; i++) image[i] = table[(i << qbits) * (qam ? 2 : 1)];
        for (size_t q = 0; q < nq; q++) image[padded(ni) + q] = table[2 * q + 1];
        for (size_t v = 0; qam && v < count; v++) {
            const float e[2] = {image[v >> qbits], image[padded(ni) + (v & (nq - 1))]};
            if (memcmp(e, &table[2 * v], sizeof e)) {
                set_error("%s: the table is no grid with %d low bits: entry %zu is not (entry %zu's real part, entry %zu's imaginary part)", name.c_str(), qbits, v,
                          v >> qbits << qbits, v & (nq - 1));
                return nullptr;
            }
        }
    }
    auto q = new_stage<DemodStage>();
    if (!q) return nullptr;
    q->qam = qam; q->soft = soft != 0; q->general = general;
    q->P = (unsigned)P; q->offset = (unsigned)offset; q->b = (int)b; q->msb = (int)msb; q->w = w;
    q->ni = (int)ni; q->nq = (int)nq; q->ibits = ibits; q->qbits = qbits;
    q->in_size = qam ? 8 : 4; q->out_size = soft ? 4 : 1;
    if (upload(q->d_table, image.data(), image.size() * sizeof(float))) return nullptr;
    return q.release();
}
