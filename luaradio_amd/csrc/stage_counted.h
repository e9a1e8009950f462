// stage_counted.h - the host pieces shared by the stages whose output count depends on the data (the sampler and clocksampler of stage_digital.h,
// the preamble sampler, Manchester decoder and Varicode decoder of stage_preamble.h, the five framers of stage_framers.h): the carve-up of a call's
// scratch and the constructor of a stage without parameters.  (What they carry between calls, and their one count read-back per call: stage_carry.h.)
// (part of liblrhip.so; included by lrhip.hip after stage_carry.h, one translation unit.  Plain host code: tools/host_carve_check.hip checks the
// scratch layouts on the CPU)
#pragma once

// ---- a call's scratch, carved into typed regions in the order they are taken, each aligned to its element type
template <class T> struct Region {
    size_t at = 0;
    T *in(const DeviceBuf &b) const { return (T *)((char *)b.p + at); }
};
struct Carve {
    struct Span { size_t at, bytes, align; };
    Span spans[8];
    int count = 0;
    size_t total = 0;                                        // what to reserve
    template <class T> Region<T> take(size_t n, size_t align = alignof(T))
    {
        const size_t at = (total + align - 1) / align * align;
        if (count < (int)(sizeof(spans) / sizeof(spans[0]))) spans[count] = Span{at, n * sizeof(T), align};
        count++;                                             // (spans is the record tools/host_carve_check.hip reads: it refuses a longer layout)
        total = at + n * sizeof(T);
        return Region<T>{at};
    }
};

// The nine layouts (members are taken in the order they are declared).  nt = tiles of the call.
struct RfScratch : Carve {
    Region<unsigned long long> mask_v; Region<int> tile_v; Region<long long> starts;
    RfScratch(unsigned long nt, unsigned long bound)
        : mask_v(take<unsigned long long>((size_t)nt * PS_WORDS)), tile_v(take<int>(nt)), starts(take<long long>(bound)) {}
};
struct EfScratch : Carve {
    Region<unsigned long long> mask_e, mask_a; Region<int> tile_e; Region<long long> starts;
    EfScratch(unsigned long nt, unsigned long bound)
        : mask_e(take<unsigned long long>((size_t)nt * PS_WORDS)), mask_a(take<unsigned long long>((size_t)nt * PS_WORDS)), tile_e(take<int>(nt)),
          starts(take<long long>(bound)) {}
};
struct AxScratch : Carve {
    Region<unsigned long long> mask_f; Region<int> tile_f; Region<long long> flags; Region<unsigned long long> segs; Region<uint8_t> valid;
    AxScratch(unsigned long nt, unsigned long max_flags, unsigned long bound)
        : mask_f(take<unsigned long long>((size_t)nt * PS_WORDS)), tile_f(take<int>(nt)), flags(take<long long>(max_flags)),
          segs(take<unsigned long long>(bound)), valid(take<uint8_t>(max_flags)) {}
};
struct PgScratch : Carve {
    Region<unsigned long long> mask_s; Region<int> tile_s;
    explicit PgScratch(unsigned long nt) : mask_s(take<unsigned long long>((size_t)nt * PS_WORDS)), tile_s(take<int>(nt)) {}
};
struct PsScratch : Carve {
    Region<unsigned long long> mask_m, mask_d; Region<int> tile_m, tile_d; Region<PsFrame> frames;    // on 16 bytes
    PsScratch(unsigned long nt, unsigned long max_frames)
        : mask_m(take<unsigned long long>((size_t)nt * PS_WORDS)), mask_d(take<unsigned long long>((size_t)nt * PS_WORDS)), tile_m(take<int>(nt)),
          tile_d(take<int>(nt)), frames(take<PsFrame>(max_frames, 16)) {}
};
struct MdScratch : Carve {
    Region<MSum> tiles; Region<int> t_state; Region<unsigned long long> t_off;
    explicit MdScratch(unsigned long nt) : tiles(take<MSum>(nt)), t_state(take<int>(nt)), t_off(take<unsigned long long>(nt)) {}
};
// tile summaries, then per tile h, rpos, kind, literal offset, previous clock, count, last bit (the 4-byte lists in slots of 8 bytes per tile)
struct ZcScratch : Carve {
    Region<HSum> tiles; Region<int> t_h; Region<long long> t_rpos; Region<int> t_kind; Region<double> t_o; Region<int> t_prev; Region<unsigned> t_cnt; Region<int> t_bit;
    explicit ZcScratch(unsigned long nt)
        : tiles(take<HSum>(nt)), t_h(take<int>(2 * (size_t)nt)), t_rpos(take<long long>(nt)), t_kind(take<int>(2 * (size_t)nt)), t_o(take<double>(nt)),
          t_prev(take<int>(2 * (size_t)nt)), t_cnt(take<unsigned>(2 * (size_t)nt)), t_bit(take<int>(2 * (size_t)nt)) {}
};
// tile maps, tile offsets, tile entry states, tile counts, then per thread "entry state, offset in the tile"
struct VcScratch : Carve {
    Region<VcMap> tiles; Region<unsigned long long> t_off; Region<int> t_state; Region<unsigned> t_cnt, t_thread;
    explicit VcScratch(unsigned long nt)
        : tiles(take<VcMap>(nt)), t_off(take<unsigned long long>(nt)), t_state(take<int>(nt)), t_cnt(take<unsigned>(nt)),
          t_thread(take<unsigned>((size_t)nt * 256)) {}
};
struct SamplerScratch : Carve {
    Region<SSum> tiles; Region<int> t_h; Region<unsigned long long> t_off;                 // (t_h in slots of 8 bytes per tile)
    explicit SamplerScratch(unsigned long nt) : tiles(take<SSum>(nt)), t_h(take<int>(2 * (size_t)nt)), t_off(take<unsigned long long>(nt)) {}
};

// ---- a stage that takes no parameters: Bit in, records of out_size bytes out
template <class Stage, int OUT_SIZE> static lrhip_stage_t *plain_create(const char *op)
{
    // (lrhip_unary_create has matched the op's name, the text in front of the ':', to the stage)
    if (const char *c = strchr(op, ':')) { set_error("%.*s: takes no parameters, got \"%s\"", (int)(c - op), op, op); return nullptr; }
    auto q = new_stage<Stage>();
    if (!q) return nullptr;
    q->in_size = 1; q->out_size = OUT_SIZE;
    if (q->reset()) return nullptr;
    return q.release();
}
