// cf_api_marks.h -- host side of the histone-mark games: mark coalitions, exact Shapley values and pair epistasis under the scale rule
// (cf_mark_*) and the donor rule (cf_mark_donor_*), the wide game and its sampled Shapley values, the window game, the fine window game.
// One MarkGame per call, built and checked by the constructor of its kind, then one of four calls on it: the given coalitions, an exact
// game (Shapley / epistasis), sampled permutations, sampled interaction indices of focal players.  Part of cf_api.hip's single translation unit: included there behind
// cf_api_attrib.h, whose chunk loop, geometry helpers and exact-game reducers it uses; not on its own.
#pragma once

// Histone-mark coalitions (cf_marks.h).  The families share everything but the options struct and the expand kernel: MarkGame is what
// the options struct says, checked.  `kind` names the table layout and, with `donor`, the kernel:
//   narrow  [words | marks_p | regions_p], one word per coalition                 k_mark_expand / k_mark_donor_expand
//   wide    [n_coal * kw words | marks_p | regions_p | extra]                       the same pair: narrow is the case kw = 1
//   window  [words | marks_p | regions_p | lo_p | hi_p | extra]                     k_mark_window_expand / k_mark_window_donor_expand
//   fine    [words | marks_p | lo_p | hi_p | start[B] | cnt_last[B] | extra]        k_mark_fine_expand / k_mark_fine_donor_expand
enum MarkKind { kMarkNarrow, kMarkWide, kMarkWindow, kMarkFine };
struct MarkGame {
    MarkKind kind = kMarkNarrow;
    int P = 0, kw = 1;                    // players; words per coalition
    const unsigned* marks = nullptr;      // host [P]
    const unsigned* regions = nullptr;    // host [P]
    float scale = 0.f;                    // the scale rule (donor == nullptr)
    const cf_mark_donor_opts* donor = nullptr;      // the donor rule
    const int* lo = nullptr;              // host [P]: player p's bins [lo, hi) -- coarsest bins (window), finest bins (fine)
    const int* hi = nullptr;
    const uint8_t* flip = nullptr;        // device [B] or null: the promoter is stored mirrored (window, fine)
    int W = 0, rc = 0;                    // the coarsest resolution's bin count and index (window)
    const cf_mark_fine_opts* fine = nullptr;      // the fine game's region and feats_out
    int rf = 0, bf = 0;                           // ... the finest resolution's index and bin size
    std::vector<unsigned> fine_words;             // ... [start[B] | cnt_last[B]]
    cf_mark_donor_opts rule_donor;                // storage: the donor's pointers of a one-struct game (mark_rule points `donor` here)
    std::vector<unsigned> fine_regions;           // storage: the one region word every player of a fine game carries (mark_check reads it)
    MarkGame() = default;
    MarkGame(const MarkGame&) = delete;      // (`donor` and `regions` may point into the game)
    void players(MarkKind k, int n, const unsigned* m, const unsigned* rg, float s) { kind = k, P = n, kw = (n + 31) / 32, marks = m, regions = rg, scale = s; }
};

// mark_check: what the entry points check alike, in front of anything launched -- the handle, the batch, riders, the options: the
// player count (at most `limit`), the player words.  `o`: whether the caller's opts pointer is non-null.
static int mark_check(cf_handle* h, const cf_batch* bt, bool o, const MarkGame& g, const char* who, int limit = kCoalMaxS) {
    if (attrib_open(h, bt, true, who)) return -1;
    if (!o) return fail("%s: null opts", who);
    const cf_config& c = h->cfg;
    const int S = c.i_max, F = c.n_feats;
    if (g.P < 1 || g.P > limit) return fail("%s: n_players = %d outside 1..%d", who, g.P, limit);
    if (!g.marks || !g.regions) return fail("%s: null player_marks / player_regions", who);
    for (int p = 0; p < g.P; ++p) {
        const unsigned pm = g.marks[p], pr = g.regions[p];
        if (!pm) return fail("%s: player_marks[%d] = 0: a player names at least one mark", who, p);
        if (!pr) return fail("%s: player_regions[%d] = 0: a player names at least one region (bit 0 the promoter, bit 1 + j pCRE slot j)", who, p);
        if (F < 32 && pm >> F) return fail("%s: player_marks[%d] = 0x%x names a mark >= n_feats = %d", who, p, pm, F);
        if (pr >> S >> 1) return fail("%s: player_regions[%d] = 0x%x names a region above i_max = %d", who, p, pr, S);
    }
    return 0;
}
// ... then the scale of the scale rule,
static int mark_game(cf_handle* h, const cf_batch* bt, const cf_mark_opts* o, MarkGame* g, const char* who) {
    if (o) g->players(kMarkNarrow, o->n_players, o->player_marks, o->player_regions, o->scale);
    if (mark_check(h, bt, o != nullptr, *g, who)) return -1;
    if (!(o->scale >= 0.f) || !std::isfinite(o->scale)) return fail("%s: scale = %g: a finite factor >= 0", who, (double)o->scale);
    return 0;
}
// ... or the donor's feature pointers of the donor rule.
static int mark_donor_game(cf_handle* h, const cf_batch* bt, const cf_mark_donor_opts* o, MarkGame* g, const char* who) {
    if (o) g->players(kMarkNarrow, o->n_players, o->player_marks, o->player_regions, 0.f), g->donor = o;
    if (mark_check(h, bt, o != nullptr, *g, who)) return -1;
    for (int r = 0; r < h->cfg.n_res; ++r)
        if (!o->donor_promoter_feats[r] || !o->donor_pcre_feats[r])
            return fail("%s: null donor_promoter_feats / donor_pcre_feats[%d]: the donor's features at every one of the model's %d resolutions", who, r, h->cfg.n_res);
    return 0;
}

// The wide game (cf_marks_wide.h): up to kMarkWideMaxP players, kw words per coalition, one options struct for both rules.
// mark_rule: which rule a one-struct game asks for -- all donor pointers null: the scale rule (g->scale, checked); all set: the donor
// rule (g->donor, filled); mixed: refused.
static int mark_rule(cf_handle* h, MarkGame* g, const float* const* don_p, const float* const* don_c, const char* who) {
    int given = 0;
    for (int r = 0; r < h->cfg.n_res; ++r) given += (don_p[r] != nullptr) + (don_c[r] != nullptr);
    if (given && given != 2 * h->cfg.n_res)
        return fail("%s: %d of the %d donor_promoter_feats / donor_pcre_feats pointers below the model's %d resolutions are null: all of them "
                    "(the scale rule) or none (the donor rule)", who, 2 * h->cfg.n_res - given, 2 * h->cfg.n_res, h->cfg.n_res);
    if (given) {
        cf_mark_donor_opts* d = &g->rule_donor;
        memset(d, 0, sizeof *d);
        for (int r = 0; r < h->cfg.n_res; ++r) d->donor_promoter_feats[r] = don_p[r], d->donor_pcre_feats[r] = don_c[r];
        g->donor = d;
        g->scale = 0.f;
    } else if (!(g->scale >= 0.f) || !std::isfinite(g->scale)) {
        return fail("%s: scale = %g: a finite factor >= 0", who, (double)g->scale);
    }
    return 0;
}
static int mark_wide_game(cf_handle* h, const cf_batch* bt, const cf_mark_wide_opts* o, MarkGame* g, const char* who) {
    if (o) g->players(kMarkWide, o->n_players, o->player_marks, o->player_regions, o->scale);
    if (mark_check(h, bt, o != nullptr, *g, who, kMarkWideMaxP)) return -1;
    return mark_rule(h, g, o->donor_promoter_feats, o->donor_pcre_feats, who);
}

// The window game (cf_mark_windows.h): the wide game's checks, then the windows against the coarsest resolution's W bins (nested bin
// counts in the scan's wording, W within the kernels' table) and the rule.  `limit`: the most players (the exact call: kCoalMaxS).
static int mark_window_game(cf_handle* h, const cf_batch* bt, const cf_mark_window_opts* o, MarkGame* g, const char* who, int limit = kMarkWideMaxP) {
    if (o) g->players(kMarkWindow, o->n_players, o->player_marks, o->player_regions, o->scale);
    if (mark_check(h, bt, o != nullptr, *g, who, limit) || coarsest(h, who, &g->rc)) return -1;
    const int W = g->W = h->cfg.n_bins[g->rc];
    if (W > kWinMaxW) return fail("%s: the coarsest resolution has W = %d bins; the window table holds at most %d", who, W, kWinMaxW);
    if (!o->player_lo || !o->player_hi) return fail("%s: null player_lo / player_hi", who);
    for (int p = 0; p < g->P; ++p) {
        const int lo = o->player_lo[p], hi = o->player_hi[p];
        if (lo < 0 || hi > W || lo >= hi)
            return fail("%s: player %d has the window [%d, %d): 0 <= lo < hi <= W = %d coarsest bins is required", who, p, lo, hi, W);
    }
    g->lo = o->player_lo, g->hi = o->player_hi, g->flip = o->flip;
    return mark_rule(h, g, o->donor_promoter_feats, o->donor_pcre_feats, who);
}

// The fine window game (cf_mark_fine.h): the wide game's checks on the players, the fine scan's on the region, the nesting, start and
// lengths (fine_tail_words, as cf_perturbation_scan_fine), then the windows and the rule.
static int mark_fine_game(cf_handle* h, const cf_batch* bt, const cf_mark_fine_opts* o, MarkGame* g, hipStream_t st, const char* who,
                          int limit = kMarkWideMaxP) {
    if (o) {
        g->fine_regions.assign((size_t)std::min(std::max(o->n_players, 1), kMarkWideMaxP), 1u);
        g->players(kMarkFine, o->n_players, o->player_marks, g->fine_regions.data(), o->scale);
    }
    if (mark_check(h, bt, o != nullptr, *g, who, limit)) return -1;
    const cf_config& c = h->cfg;
    const int nres = c.n_res, S = c.i_max, B = bt->B;
    if (o->region < 0 || o->region > S) return fail("%s: region = %d outside [0, i_max = %d]", who, o->region, S);
    int rc = 0;      // (nested bin counts, in the scan's wording: the zoom starts from coarse windows)
    if (coarsest(h, who, &rc) || finest(h, who, &g->rf)) return -1;
    const int rf = g->rf, Lf = c.n_bins[rf];
    if (Lf > kFineMaxL) return fail("%s: the finest resolution has n_bins[%d] = %d bins; the window table holds at most %d", who, rf, Lf, kFineMaxL);
    for (int r = nres; r < kMaxRes; ++r)
        if (o->feats_out[r]) return fail("%s: feats_out[%d]: the model has %d resolutions", who, r, nres);
    if (!o->player_lo || !o->player_hi) return fail("%s: null player_lo / player_hi", who);
    for (int p = 0; p < g->P; ++p) {
        const int lo = o->player_lo[p], hi = o->player_hi[p];
        if (lo < 0 || lo >= hi) return fail("%s: player %d has the window [%d, %d): 0 <= lo < hi finest bins is required", who, p, lo, hi);
    }
    for (int b = 0; o->start && b < B; ++b)
        if (o->start[b] < 0) return fail("%s: start[%d] = %d: a finest genomic bin >= 0", who, b, o->start[b]);
    g->lo = o->player_lo, g->hi = o->player_hi, g->flip = o->flip, g->fine = o, g->bf = c.binsizes[rf];
    if (mark_rule(h, g, o->donor_promoter_feats, o->donor_pcre_feats, who)) return -1;
    g->fine_words.resize(2 * (size_t)B);
    return fine_tail_words(h, bt, o->region, rf, o->start, o->lengths, st, who, g->fine_words.data());
}

// The n_coal * kw coalition words (validated) and the player words into the workspace's word table, in the layout of the game's kind
// (above), with room for `extra` words behind them.
static int mark_player_words(const MarkGame& g) { return g.kind == kMarkFine ? 3 * g.P + (int)g.fine_words.size() : (g.kind == kMarkWindow ? 4 : 2) * g.P; }
static int mark_upload(cf_handle* h, const MarkGame& g, const uint32_t* keep, int n_coal, size_t extra, hipStream_t st, const char* who) {
    const int P = g.P, kw = g.kw;
    if (n_coal < 1) return fail("%s: n_coal = %d: at least 1 coalition", who, n_coal);
    if (!keep) return fail("%s: null keep", who);
    if (P & 31)
        for (int k = 0; k < n_coal; ++k) {
            const uint32_t last = keep[(size_t)k * kw + kw - 1];
            if (!(last >> (P & 31))) continue;
            if (g.kind == kMarkNarrow) return fail("%s: keep[%d] = 0x%x names a player >= n_players = %d", who, k, last, P);
            return fail("%s: keep[%d] (word %d = 0x%x) names a player >= n_players = %d", who, k, kw - 1, last, P);
        }
    const size_t nw = (size_t)n_coal * kw;
    if (attrib_ws(h, who) || h->aw.words.need(nw + mark_player_words(g) + extra, 256, who)) return -1;
    unsigned* tab = h->aw.words;
    HIP_TRY(hipMemcpyAsync(tab, keep, nw * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tab + nw, g.marks, P * sizeof(unsigned), hipMemcpyHostToDevice, st));
    unsigned* at = tab + nw + P;
    if (g.kind != kMarkFine) {
        HIP_TRY(hipMemcpyAsync(at, g.regions, P * sizeof(unsigned), hipMemcpyHostToDevice, st));
        at += P;
    }
    if (g.lo) {
        HIP_TRY(hipMemcpyAsync(at, g.lo, P * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(at + P, g.hi, P * sizeof(int), hipMemcpyHostToDevice, st));
        at += 2 * P;
    }
    if (!g.fine_words.empty()) HIP_TRY(hipMemcpyAsync(at, g.fine_words.data(), g.fine_words.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    return 0;
}

// The B * n_coal rows of a mark-coalition call (gene-major; row (b, k) is coalition k of the table mark_upload wrote), every row
// through the whole forward: chunk_forward with the expand kernel of the game's kind and rule, on the argument struct of that kind.
// k_attc2 takes as many regions per workgroup as for the caller's B genes (ag_genes), as scan_region_rows: the result does not depend
// on max_batch.  `own`: a table of n_coal coalitions PER GENE at own + b * stride (the back-selection), the player words staying where
// mark_upload put them behind `n_up` shared coalitions; null: the shared table mark_upload wrote, n_coal coalitions.
static int mark_rows(cf_handle* h, const cf_batch* bt, const MarkGame& g, int n_coal, float* logits, hipStream_t st, const unsigned* own = nullptr,
                     long long stride = 0, int n_up = 0) {
    const cf_config& c = h->cfg;
    const int nres = c.n_res, B = bt->B, P = g.P;
    MarkExpandArgs ea;      // what every kind reads
    memset(&ea, 0, sizeof ea);
    cf_batch cb;            // the chunk's batch: the rows' copies
    chunk_rows(h, bt, &ea.rows, &cb);
    for (int r = 0; r < nres; ++r) {
        ea.pf_in[r] = bt->promoter_feats[r];
        ea.cf_in[r] = bt->pcre_feats[r];
        ea.pf_out[r] = h->aw.row[r];
        ea.cf_out[r] = h->aw.row[kMaxRes + r];
    }
    ea.freq_in = bt->interaction_freq;
    ea.freq_out = h->aw.row[2 * kMaxRes];
    ea.words = own ? own : (const unsigned*)h->aw.words;
    ea.word_stride = own ? stride : 0;
    ea.players = h->aw.words + (size_t)(own ? n_up : n_coal) * g.kw;
    ea.scale = g.scale;
    ea.n_coal = n_coal, ea.P = P, ea.F = c.n_feats;
    auto donor_feats = [&](const float** pf, const float** cf) {
        for (int r = 0; g.donor && r < nres; ++r) pf[r] = g.donor->donor_promoter_feats[r], cf[r] = g.donor->donor_pcre_feats[r];
    };
    // the chunk loop on `d` (the donor rule's struct, its first member `a` the scale rule's, whose first member is `m`): kernel kd or k
    const long long launches0 = g_launches;
    auto run = [&](auto kd, const char* nd, auto k, const char* nk, auto& d, auto& a, MarkExpandArgs& m) {
        const int rv = chunk_forward(h, &cb, (long long)B * n_coal, logits, true, B, st, [&](long long g0, int n) {
            m.g0 = g0;
            const dim3 grid(n, nres, kMarkSlices);
            return g.donor ? launch_expand(kd, nd, grid, kIgxThreads, d, st) : launch_expand(k, nk, grid, kIgxThreads, a, st);
        });
        h->x0_fwd = false;
        forward_counted(h, launches0);
        return rv ? -1 : 0;
    };
    if (g.kind == kMarkFine) {      // ea with the region's centre mask rows, start, the tail counts and feats_out
        MarkFineDonorArgs fd;
        memset(&fd, 0, sizeof fd);
        fd.w.m = ea;
        donor_feats(fd.pf_don, fd.cf_don);
        for (int r = 0; r < nres; ++r) {
            region_mask_row(bt, g.fine->region, r, c.i_max, &fd.w.rm_in[r], &fd.w.rm_stride[r]);
            fd.w.feats_out[r] = g.fine->feats_out[r];
        }
        fd.w.start = reinterpret_cast<const int*>(ea.players) + 3 * P;
        fd.w.cnt_last = fd.w.start + B;
        fd.w.flip = g.flip;
        fd.w.rf = g.rf, fd.w.bf = g.bf, fd.w.region = g.fine->region;
        return run(k_mark_fine_donor_expand, "k_mark_fine_donor_expand", k_mark_fine_expand, "k_mark_fine_expand", fd, fd.w, fd.w.m);
    }
    if (g.kind == kMarkWindow) {      // ea with the promoter's centre mask rows, flip and the coarsest resolution
        MarkWindowDonorArgs wd;
        memset(&wd, 0, sizeof wd);
        wd.w.m = ea;
        donor_feats(wd.pf_don, wd.cf_don);
        for (int r = 0; r < nres; ++r) wd.w.pmc[r] = bt->promoter_mask_row[r];
        wd.w.flip = g.flip;
        wd.w.W = g.W, wd.w.rc = g.rc;
        return run(k_mark_window_donor_expand, "k_mark_window_donor_expand", k_mark_window_expand, "k_mark_window_expand", wd, wd.w, wd.w.m);
    }
    MarkDonorArgs da;
    memset(&da, 0, sizeof da);
    da.m = ea;
    donor_feats(da.pf_don, da.cf_don);
    return run(k_mark_donor_expand, "k_mark_donor_expand", k_mark_expand, "k_mark_expand", da, da.m, da.m);
}

// The three calls on a checked game: the given coalitions;
static int mark_coalitions_impl(cf_handle* h, const cf_batch* bt, const MarkGame& g, const uint32_t* keep, int n_coal, float* logits, void* stream,
                                const char* who) {
    if (!logits) return fail("%s: null logits", who);
    hipStream_t st = (hipStream_t)stream;
    if (mark_upload(h, g, keep, n_coal, 0, st, who)) return -1;
    return mark_rows(h, bt, g, n_coal, logits, st);
}
// an exact game -- all 2^P coalitions and k_shapley, the pair-deletion coalitions and k_epistasis, or all 2^P coalitions and
// k_shapley_pairs (with k_shapley if `phi` is given), with S = P (all_words / launch_shapley, pair_words / launch_epistasis,
// launch_interactions: cf_api_attrib.h) -- through mark_upload + mark_rows;
enum MarkExact { kExactShapley, kExactEpistasis, kExactInteractions };
static int mark_exact_impl(cf_handle* h, const cf_batch* bt, const MarkGame& g, MarkExact what, float* out, float* logits_rows, void* stream,
                           const char* who, int index = 0, float* phi = nullptr) {
    if (what == kExactInteractions) {
        if (interactions_check(index, g.P, out, who)) return -1;
    } else if (!out) {
        return fail(what == kExactEpistasis ? "%s: null eps" : "%s: null phi", who);
    }
    const std::vector<uint32_t> keep = what == kExactEpistasis ? pair_words(g.P) : all_words(g.P);
    const int R = (int)keep.size();
    float* rows = coalition_out_rows(h, logits_rows, R, who);
    if (!rows) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (mark_upload(h, g, keep.data(), R, 0, st, who) || mark_rows(h, bt, g, R, rows, st)) return -1;
    if (what == kExactInteractions) return launch_interactions(h, bt->B, g.P, index, rows, out, phi, st);
    return what == kExactEpistasis ? launch_epistasis(h, bt->B, g.P, rows, out, st) : launch_shapley(h, bt->B, g.P, rows, out, st);
}
// the prefix rows of n_perm permutations through mark_upload + mark_rows (column 0 nobody, column 1 everybody, column
// 2 + q (P - 1) + (k - 1) the first k players of permutation q), then k_perm_shapley on the inverse permutations, which travel as bytes
// behind the player words.  `g`: a checked game of a kind with kw words per coalition (wide, window, fine).
static int perm_ranks(const uint8_t* perms, int n_perm, int P, std::vector<uint8_t>* rank, const char* who) {      // the inverses, checked
    rank->assign((size_t)n_perm * P, 0xFF);
    for (int q = 0; q < n_perm; ++q) {
        const uint8_t* pi = perms + (size_t)q * P;
        uint8_t* rk = rank->data() + (size_t)q * P;
        for (int k = 0; k < P; ++k) {
            if (pi[k] >= P || rk[pi[k]] != 0xFF) return fail("%s: perms[%d] is not a permutation of 0..%d (position %d holds %d)", who, q, P - 1, k, (int)pi[k]);
            rk[pi[k]] = (uint8_t)k;
        }
    }
    return 0;
}
static void prefix_words(const uint8_t* perms, int n_perm, int P, int kw, uint32_t* keep) {      // the 2 + n_perm (P - 1) leading rows, zeroed
    std::vector<uint32_t> cur(kw);
    for (int p = 0; p < P; ++p) keep[kw + (p >> 5)] |= 1u << (p & 31);      // column 1: everybody
    for (int q = 0; q < n_perm; ++q) {
        const uint8_t* pi = perms + (size_t)q * P;
        std::fill(cur.begin(), cur.end(), 0u);
        for (int k = 1; k < P; ++k) {
            cur[pi[k - 1] >> 5] |= 1u << (pi[k - 1] & 31);
            memcpy(&keep[(2 + (size_t)q * (P - 1) + (k - 1)) * kw], cur.data(), kw * sizeof(uint32_t));
        }
    }
}
// k_perm_shapley on the prefix rows that lead a table of `stride` rows per gene (0: the prefix rows are the table)
static int launch_perm_shapley(cf_handle* h, int B, int P, int n_out, int n_perm, const float* rows, size_t stride, const uint8_t* rank_at, float* phi, float* se,
                               hipStream_t st) {
    PermShapleyArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.v = rows, pa.rank = rank_at, pa.phi = phi, pa.se = se;
    pa.n = (float)n_perm, pa.nn1 = (float)((double)n_perm * (n_perm - 1));
    pa.P = P, pa.n_perm = n_perm, pa.n_out = n_out, pa.stride = stride;
    hipLaunchKernelGGL(k_perm_shapley, dim3(B, P), dim3(kShapThreads), 0, st, pa);
    LAUNCH_CHECK("k_perm_shapley");
    forward_one_more(h);
    return 0;
}
static int mark_sampled_impl(cf_handle* h, const cf_batch* bt, const MarkGame& g, const uint8_t* perms, int n_perm, float* phi, float* se,
                             float* logits_rows, void* stream, const char* who) {
    if (!phi) return fail("%s: null phi", who);
    if (!perms) return fail("%s: null perms", who);
    if (n_perm < 1) return fail("%s: n_perm = %d: at least 1 permutation", who, n_perm);
    const int P = g.P, kw = g.kw;
    const long long R64 = 2 + (long long)n_perm * (P - 1);
    if (R64 * kw > (1ll << 30)) return fail("%s: n_perm = %d: %lld rows per gene; at most 2^30 coalition words", who, n_perm, R64);
    const int R = (int)R64;
    std::vector<uint8_t> rank;
    if (perm_ranks(perms, n_perm, P, &rank, who)) return -1;
    std::vector<uint32_t> keep((size_t)R * kw, 0u);
    prefix_words(perms, n_perm, P, kw, keep.data());
    float* rows = coalition_out_rows(h, logits_rows, R, who);
    if (!rows) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (mark_upload(h, g, keep.data(), R, (rank.size() + 3) / 4, st, who)) return -1;
    uint8_t* rank_at = reinterpret_cast<uint8_t*>((unsigned*)h->aw.words + (size_t)R * kw + mark_player_words(g));
    HIP_TRY(hipMemcpyAsync(rank_at, rank.data(), rank.size(), hipMemcpyHostToDevice, st));
    if (mark_rows(h, bt, g, R, rows, st)) return -1;
    return launch_perm_shapley(h, bt->B, P, h->cfg.n_out, n_perm, rows, 0, rank_at, phi, se, st);
}

// Sampled pairwise interaction indices of focal players (cf_mark_pairs.h).  FocalTable: what the host builds from the orders and the
// focal players -- the inverse permutations, the R coalitions (kw words each: the prefix rows of mark_sampled_impl, then per focal player
// {i}, everybody but i, and per order the rows T_k + i, k = 1 .. r - 1, and T_k, k = r + 1 .. P - 2), and col[f, q, k, {without, with}].
struct FocalTable {
    std::vector<uint8_t> rank;
    std::vector<uint32_t> keep, col;
    long long R = 0;
};
// What the sampled-interactions calls check beside their game, then the table.  Refused by name: null inter / perms / focal, n_perm < 1,
// n_focal outside 1..P, index, P < 2, a focal index outside 0..P-1 or repeated (its position is named), a row of perms that is no
// permutation, more than 2^30 coalition words.
static int focal_table(int P, const uint8_t* perms, int n_perm, const int* focal, int n_focal, int index, const float* inter, const float* phi,
                       const float* phi_se, FocalTable* t, const char* who) {
    if (interactions_check(index, P, inter, who)) return -1;
    if (phi_se && !phi) return fail("%s: phi_se without phi", who);
    if (!perms) return fail("%s: null perms", who);
    if (n_perm < 1) return fail("%s: n_perm = %d: at least 1 permutation", who, n_perm);
    if (!focal) return fail("%s: null focal", who);
    if (n_focal < 1 || n_focal > P) return fail("%s: n_focal = %d outside 1..%d", who, n_focal, P);
    for (int f = 0; f < n_focal; ++f) {
        if (focal[f] < 0 || focal[f] >= P) return fail("%s: focal[%d] = %d outside 0..%d", who, f, focal[f], P - 1);
        for (int e = 0; e < f; ++e)
            if (focal[e] == focal[f]) return fail("%s: focal[%d] = %d repeats focal[%d]", who, f, focal[f], e);
    }
    if (perm_ranks(perms, n_perm, P, &t->rank, who)) return -1;
    const int kw = (P + 31) / 32;
    auto extra = [&](int r) { return r == 0 || r == P - 1 ? P - 2 : P - 3; };      // the rows of one (focal, order) that are no prefix
    long long R = 2 + (long long)n_perm * (P - 1);
    for (int f = 0; f < n_focal; ++f) {
        R += 2;
        for (int q = 0; q < n_perm; ++q) R += extra(t->rank[(size_t)q * P + focal[f]]);
    }
    if (R * kw > (1ll << 30)) return fail("%s: n_perm = %d, n_focal = %d: %lld rows per gene; at most 2^30 coalition words", who, n_perm, n_focal, R);
    t->R = R;
    t->keep.assign((size_t)R * kw, 0u);
    t->col.assign((size_t)n_focal * n_perm * P * 2, 0u);
    prefix_words(perms, n_perm, P, kw, t->keep.data());
    std::vector<uint32_t> cur(kw);
    auto put = [&](std::vector<uint32_t>& w, int p) { w[p >> 5] |= 1u << (p & 31); };
    size_t row = 2 + (size_t)n_perm * (P - 1);
    auto emit = [&]() {      // (a row past the count is not written: the count is checked below)
        if (row < (size_t)R) memcpy(&t->keep[row * kw], cur.data(), kw * sizeof(uint32_t));
        return (uint32_t)row++;
    };
    for (int f = 0; f < n_focal; ++f) {
        const int i = focal[f];
        std::fill(cur.begin(), cur.end(), 0u);
        put(cur, i);
        const uint32_t alone = emit();
        memcpy(cur.data(), &t->keep[kw], kw * sizeof(uint32_t));
        cur[i >> 5] &= ~(1u << (i & 31));
        const uint32_t without = emit();
        for (int q = 0; q < n_perm; ++q) {
            const uint8_t* pi = perms + (size_t)q * P;
            const int r = t->rank[(size_t)q * P + i];
            uint32_t* c = &t->col[((size_t)f * n_perm + q) * P * 2];
            auto prefix = [&](int k) { return (uint32_t)(2 + (size_t)q * (P - 1) + (k - 1)); };      // the first k of pi, 1 <= k <= P - 1
            // (a prefix of pi where there is one: the diagonal then reads the very rows k_perm_shapley reads, on any table)
            c[0] = 0, c[1] = r == 0 ? prefix(1) : alone;
            c[2 * (P - 1)] = r == P - 1 ? prefix(P - 1) : without, c[2 * (P - 1) + 1] = 1;
            std::fill(cur.begin(), cur.end(), 0u);
            put(cur, i);
            for (int k = 1; k <= P - 2; ++k) {      // T_k + i: an own row in front of i's position, the prefix pi[:k + 1] from there on
                if (k < r) put(cur, pi[k - 1]);
                c[2 * k + 1] = k < r ? emit() : prefix(k + 1);
            }
            std::fill(cur.begin(), cur.end(), 0u);
            for (int k = 0; k <= r && k < P; ++k)
                if (k != r) put(cur, pi[k]);
            for (int k = 1; k <= P - 2; ++k) {      // T_k: the prefix pi[:k] up to i's position, an own row behind it (pi[:k + 1] less i)
                if (k > r) put(cur, pi[k]);
                c[2 * k] = k > r ? emit() : prefix(k);
            }
        }
    }
    if ((long long)row != R) return fail("%s: internal: %zu rows built, %lld counted", who, row, R);
    return 0;
}
// k_perm_pairs on a table in FocalTable's layout, rank and col on the device, and k_perm_shapley on its leading rows if phi is given.
static int launch_perm_pairs(cf_handle* h, int B, int P, int n_out, int n_perm, const int* focal, int n_focal, int index, const float* rows, size_t R,
                             const uint8_t* rank_at, const unsigned* col_at, float* inter, float* se, float* phi, float* phi_se, hipStream_t st) {
    PermPairsArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.v = rows, pa.rank = rank_at, pa.col = col_at, pa.inter = inter, pa.se = se, pa.R = R;
    pa.n = (float)n_perm, pa.nn1 = (float)((double)n_perm * (n_perm - 1));
    pa.P = P, pa.n_perm = n_perm, pa.n_out = n_out, pa.n_focal = n_focal, pa.sti = index == CF_INTERACTION_STI;
    for (int f = 0; f < n_focal; ++f) pa.focal[f] = (uint8_t)focal[f];
    for (int a = 0; a < P - 1; ++a) pa.w[a] = (float)(2.0 * (P - 1 - a) / P);
    hipLaunchKernelGGL(k_perm_pairs, dim3(B, n_focal * P), dim3(kShapThreads), 0, st, pa);
    LAUNCH_CHECK("k_perm_pairs");
    forward_one_more(h);
    return phi ? launch_perm_shapley(h, B, P, n_out, n_perm, rows, R, rank_at, phi, phi_se, st) : 0;
}
// rank (bytes) and col behind `at` words of the word table, which has room for them
static int focal_upload(cf_handle* h, const FocalTable& t, size_t at, const uint8_t** rank_at, const unsigned** col_at, hipStream_t st) {
    unsigned* tab = (unsigned*)h->aw.words + at;
    HIP_TRY(hipMemcpyAsync(tab, t.rank.data(), t.rank.size(), hipMemcpyHostToDevice, st));
    unsigned* c = tab + (t.rank.size() + 3) / 4;
    HIP_TRY(hipMemcpyAsync(c, t.col.data(), t.col.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    *rank_at = reinterpret_cast<const uint8_t*>(tab), *col_at = c;
    return 0;
}
// The call on a checked game of a kind with kw words per coalition (wide, window, fine): the R rows through mark_upload + mark_rows,
// then the reducers.
static int mark_pairs_sampled_impl(cf_handle* h, const cf_batch* bt, const MarkGame& g, const uint8_t* perms, int n_perm, const int* focal,
                                   int n_focal, int index, float* inter, float* se, float* phi, float* phi_se, float* logits_rows, void* stream,
                                   const char* who) {
    FocalTable t;
    if (focal_table(g.P, perms, n_perm, focal, n_focal, index, inter, phi, phi_se, &t, who)) return -1;
    const int R = (int)t.R;
    float* rows = coalition_out_rows(h, logits_rows, R, who);
    if (!rows) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (mark_upload(h, g, t.keep.data(), R, (t.rank.size() + 3) / 4 + t.col.size(), st, who)) return -1;
    const uint8_t* rank_at;
    const unsigned* col_at;
    if (focal_upload(h, t, (size_t)R * g.kw + mark_player_words(g), &rank_at, &col_at, st) || mark_rows(h, bt, g, R, rows, st)) return -1;
    return launch_perm_pairs(h, bt->B, g.P, h->cfg.n_out, n_perm, focal, n_focal, index, rows, (size_t)R, rank_at, col_at, inter, se, phi, phi_se, st);
}
// The operator on a caller's table in that layout: no batch, no chunk workspace, nothing of the handle but the word table.
extern "C" int cf_perm_interactions_from_rows(cf_handle* h, const float* rows, int B, int P, int n_out, const uint8_t* perms, int n_perm,
                                              const int* focal, int n_focal, int index, float* inter, float* se, float* phi, float* phi_se,
                                              void* stream) {
    const char* who = "cf_perm_interactions_from_rows";
    if (!h) return fail("%s: null handle", who);
    if (!rows) return fail("%s: null rows", who);
    if (B < 1) return fail("%s: B = %d: at least 1 gene", who, B);
    if (P > kMarkWideMaxP) return fail("%s: P = %d outside 2..%d", who, P, kMarkWideMaxP);
    if (n_out < 1) return fail("%s: n_out = %d: at least 1 output", who, n_out);
    FocalTable t;
    if (focal_table(P, perms, n_perm, focal, n_focal, index, inter, phi, phi_se, &t, who)) return -1;
    if (h->aw.words.need((t.rank.size() + 3) / 4 + t.col.size(), 256, who)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* rank_at;
    const unsigned* col_at;
    if (focal_upload(h, t, 0, &rank_at, &col_at, st)) return -1;
    h->n_fwd = 0;
    return launch_perm_pairs(h, B, P, n_out, n_perm, focal, n_focal, index, rows, (size_t)t.R, rank_at, col_at, inter, se, phi, phi_se, st);
}

// Greedy player selection on a checked game (cf_backselect.h).  What the calls check beside their game, by name: null opts / outputs,
// mode, direction, target, frac, the four required outputs.
static int backselect_check(const cf_backselect_opts* o, const cf_backselect_out* out, int n_out, const char* who) {
    if (!o) return fail("%s: null backselect opts", who);
    if (!out) return fail("%s: null outputs", who);
    if (o->mode != CF_BACKSELECT_BACKWARD && o->mode != CF_BACKSELECT_FORWARD)
        return fail("%s: mode = %d: CF_BACKSELECT_BACKWARD (%d) or CF_BACKSELECT_FORWARD (%d)", who, o->mode, CF_BACKSELECT_BACKWARD, CF_BACKSELECT_FORWARD);
    if (o->direction < -1 || o->direction > 1) return fail("%s: direction = %d: 0 (from the two end rows), +1 or -1", who, o->direction);
    if (o->target < 0 || o->target >= n_out) return fail("%s: target = %d outside [0, n_out = %d)", who, o->target, n_out);
    if (!std::isfinite(o->frac)) return fail("%s: frac = %g: a finite number", who, (double)o->frac);
    if (!out->order || !out->values || !out->size || !out->subset) return fail("%s: null order / values / size / subset", who);
    return 0;
}
// The two end rows (nobody, everybody: the shared table mark_upload wrote), then per round t = 0 .. P - 2 one k_backselect_step -- the
// pick among the previous round's rows and the gene's P - t candidate words -- and the B (P - t) rows of the round through mark_rows on
// the per-gene table; one more k_backselect_step for the last pick, then k_backselect_finish.  Launches, with n_fwd those of
// cf_forward(save = 0) and M = max_batch:
//   P + 1 + (1 + n_fwd) (ceil(2 B / M) + sum over t = 0 .. P - 2 of ceil(B (P - t) / M))
// cur [B, kw], the candidates [B, P, kw] and s_b [B] live behind the player words in the word table; the rows in the caller's buffer or
// the handle's own.  The host sees no logit: no synchronisation, no copy back.
static int mark_backselect_impl(cf_handle* h, const cf_batch* bt, const MarkGame& g, const cf_backselect_opts* o, const cf_backselect_out* out,
                                void* stream, const char* who) {
    const int B = bt->B, P = g.P, kw = g.kw, n_out = h->cfg.n_out;
    if (backselect_check(o, out, n_out, who)) return -1;
    if (g.fine)
        for (int r = 0; r < kMaxRes; ++r)
            if (g.fine->feats_out[r]) return fail("%s: feats_out[%d]: the rounds have different row counts; the back-selection writes no features", who, r);
    float* rows = coalition_out_rows(h, out->rows, 1 + (long long)P * (P + 1) / 2, who);
    if (!rows) return -1;
    hipStream_t st = (hipStream_t)stream;
    std::vector<uint32_t> ends(2 * (size_t)kw, 0u);
    for (int p = 0; p < P; ++p) ends[kw + (p >> 5)] |= 1u << (p & 31);
    if (mark_upload(h, g, ends.data(), 2, (size_t)B * kw * (1 + P) + B, st, who)) return -1;
    const long long launches0 = g_launches;
    if (mark_rows(h, bt, g, 2, rows, st)) return -1;
    BackselectArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.ends = rows;
    sa.cur = (unsigned*)h->aw.words + 2 * kw + mark_player_words(g);
    sa.cand = sa.cur + (size_t)B * kw;
    sa.dir = reinterpret_cast<int*>(sa.cand + (size_t)B * P * kw);
    sa.order = out->order, sa.values = out->values, sa.dir_out = out->direction;
    sa.P = P, sa.kw = kw, sa.n_out = n_out, sa.mode = o->mode, sa.target = o->target, sa.direction = o->direction;
    float* at = rows + (size_t)B * 2 * n_out;
    for (int t = 0; t < P; ++t) {
        sa.t = t;
        hipLaunchKernelGGL(k_backselect_step, dim3(B), dim3(kBsThreads), 0, st, sa);
        LAUNCH_CHECK("k_backselect_step");
        if (t == P - 1) break;
        if (mark_rows(h, bt, g, P - t, at, st, sa.cand, (long long)P * kw, 2)) return -1;
        sa.prev = at;
        at += (size_t)B * (P - t) * n_out;
    }
    BackselectFinishArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.ends = rows, fa.dir = sa.dir, fa.order = out->order, fa.values = out->values, fa.size = out->size, fa.subset = out->subset;
    fa.threshold = o->threshold, fa.thr_out = out->threshold, fa.frac = o->frac;
    fa.P = P, fa.kw = kw, fa.n_out = n_out, fa.mode = o->mode, fa.target = o->target;
    hipLaunchKernelGGL(k_backselect_finish, dim3(B), dim3(kBsThreads), 0, st, fa);
    LAUNCH_CHECK("k_backselect_finish");
    forward_counted(h, launches0);
    return 0;
}
// The same selection on a caller's table [B, 2^P, n_out]: no batch, no workspace, nothing of the handle is read and no activation written.
extern "C" int cf_backselect_from_rows(cf_handle* h, const float* rows, int B, int P, int n_out, const cf_backselect_opts* o, const cf_backselect_out* out,
                                       void* stream) {
    const char* who = "cf_backselect_from_rows";
    if (!h) return fail("%s: null handle", who);
    if (!rows) return fail("%s: null rows", who);
    if (B < 1) return fail("%s: B = %d: at least 1 gene", who, B);
    if (P < 1 || P > kCoalMaxS) return fail("%s: P = %d outside 1..%d", who, P, kCoalMaxS);
    if (n_out < 1) return fail("%s: n_out = %d: at least 1 output", who, n_out);
    if (backselect_check(o, out, n_out, who)) return -1;
    BackselectTableArgs ta;
    memset(&ta, 0, sizeof ta);
    ta.v = rows, ta.order = out->order, ta.values = out->values, ta.size = out->size, ta.subset = out->subset;
    ta.threshold = o->threshold, ta.thr_out = out->threshold, ta.dir_out = out->direction, ta.frac = o->frac;
    ta.P = P, ta.n_out = n_out, ta.mode = o->mode, ta.target = o->target, ta.direction = o->direction;
    h->n_fwd = 0;
    hipLaunchKernelGGL(k_backselect_table, dim3(B), dim3(kBsTableThreads), 0, (hipStream_t)stream, ta);
    LAUNCH_CHECK("k_backselect_table");
    forward_one_more(h);
    return 0;
}
// one entry point per kind with kw words per coalition (the narrow game is cf_mark_backselect with at most 32 players)
extern "C" int cf_mark_backselect(cf_handle* h, const cf_batch* bt, const cf_mark_wide_opts* o, const cf_backselect_opts* bo, const cf_backselect_out* out,
                                  void* stream) {
    const char* who = "cf_mark_backselect";
    MarkGame g;
    return mark_wide_game(h, bt, o, &g, who) ? -1 : mark_backselect_impl(h, bt, g, bo, out, stream, who);
}
extern "C" int cf_mark_window_backselect(cf_handle* h, const cf_batch* bt, const cf_mark_window_opts* o, const cf_backselect_opts* bo,
                                         const cf_backselect_out* out, void* stream) {
    const char* who = "cf_mark_window_backselect";
    MarkGame g;
    return mark_window_game(h, bt, o, &g, who) ? -1 : mark_backselect_impl(h, bt, g, bo, out, stream, who);
}
extern "C" int cf_mark_fine_backselect(cf_handle* h, const cf_batch* bt, const cf_mark_fine_opts* o, const cf_backselect_opts* bo,
                                       const cf_backselect_out* out, void* stream) {
    const char* who = "cf_mark_fine_backselect";
    MarkGame g;
    return mark_fine_game(h, bt, o, &g, (hipStream_t)stream, who) ? -1 : mark_backselect_impl(h, bt, g, bo, out, stream, who);
}

// The entry points: the game of the family, then its call.  The scale rule's one-word game;
extern "C" int cf_mark_coalitions(cf_handle* h, const cf_batch* bt, const cf_mark_opts* o, const uint32_t* keep, int n_coal, float* logits,
                                  void* stream) {
    const char* who = "cf_mark_coalitions";
    MarkGame g;
    return mark_game(h, bt, o, &g, who) ? -1 : mark_coalitions_impl(h, bt, g, keep, n_coal, logits, stream, who);
}
extern "C" int cf_mark_shapley(cf_handle* h, const cf_batch* bt, const cf_mark_opts* o, float* phi, float* logits_all, void* stream) {
    const char* who = "cf_mark_shapley";
    MarkGame g;
    return mark_game(h, bt, o, &g, who) ? -1 : mark_exact_impl(h, bt, g, kExactShapley, phi, logits_all, stream, who);
}
extern "C" int cf_mark_epistasis(cf_handle* h, const cf_batch* bt, const cf_mark_opts* o, float* eps, float* logits_pairs, void* stream) {
    const char* who = "cf_mark_epistasis";
    MarkGame g;
    return mark_game(h, bt, o, &g, who) ? -1 : mark_exact_impl(h, bt, g, kExactEpistasis, eps, logits_pairs, stream, who);
}
extern "C" int cf_mark_shapley_interactions(cf_handle* h, const cf_batch* bt, const cf_mark_opts* o, int index, float* inter, float* phi,
                                            float* logits_all, void* stream) {
    const char* who = "cf_mark_shapley_interactions";
    MarkGame g;
    return mark_game(h, bt, o, &g, who) ? -1 : mark_exact_impl(h, bt, g, kExactInteractions, inter, logits_all, stream, who, index, phi);
}

// the donor family: an absent mark takes the donor's bits (k_mark_donor_expand); everything else as above;
extern "C" int cf_mark_donor_coalitions(cf_handle* h, const cf_batch* bt, const cf_mark_donor_opts* o, const uint32_t* keep, int n_coal,
                                        float* logits, void* stream) {
    const char* who = "cf_mark_donor_coalitions";
    MarkGame g;
    return mark_donor_game(h, bt, o, &g, who) ? -1 : mark_coalitions_impl(h, bt, g, keep, n_coal, logits, stream, who);
}
extern "C" int cf_mark_donor_shapley(cf_handle* h, const cf_batch* bt, const cf_mark_donor_opts* o, float* phi, float* logits_all, void* stream) {
    const char* who = "cf_mark_donor_shapley";
    MarkGame g;
    return mark_donor_game(h, bt, o, &g, who) ? -1 : mark_exact_impl(h, bt, g, kExactShapley, phi, logits_all, stream, who);
}
extern "C" int cf_mark_donor_epistasis(cf_handle* h, const cf_batch* bt, const cf_mark_donor_opts* o, float* eps, float* logits_pairs, void* stream) {
    const char* who = "cf_mark_donor_epistasis";
    MarkGame g;
    return mark_donor_game(h, bt, o, &g, who) ? -1 : mark_exact_impl(h, bt, g, kExactEpistasis, eps, logits_pairs, stream, who);
}
extern "C" int cf_mark_donor_shapley_interactions(cf_handle* h, const cf_batch* bt, const cf_mark_donor_opts* o, int index, float* inter, float* phi,
                                                  float* logits_all, void* stream) {
    const char* who = "cf_mark_donor_shapley_interactions";
    MarkGame g;
    return mark_donor_game(h, bt, o, &g, who) ? -1 : mark_exact_impl(h, bt, g, kExactInteractions, inter, logits_all, stream, who, index, phi);
}

// the wide game;
extern "C" int cf_mark_coalitions_wide(cf_handle* h, const cf_batch* bt, const cf_mark_wide_opts* o, const uint32_t* keep, int n_coal, float* logits,
                                       void* stream) {
    const char* who = "cf_mark_coalitions_wide";
    MarkGame g;
    return mark_wide_game(h, bt, o, &g, who) ? -1 : mark_coalitions_impl(h, bt, g, keep, n_coal, logits, stream, who);
}
extern "C" int cf_mark_shapley_sampled(cf_handle* h, const cf_batch* bt, const cf_mark_wide_opts* o, const uint8_t* perms, int n_perm, float* phi,
                                       float* se, float* logits_rows, void* stream) {
    const char* who = "cf_mark_shapley_sampled";
    MarkGame g;
    return mark_wide_game(h, bt, o, &g, who) ? -1 : mark_sampled_impl(h, bt, g, perms, n_perm, phi, se, logits_rows, stream, who);
}

// the window game;
extern "C" int cf_mark_window_coalitions(cf_handle* h, const cf_batch* bt, const cf_mark_window_opts* o, const uint32_t* keep, int n_coal,
                                         float* logits, void* stream) {
    const char* who = "cf_mark_window_coalitions";
    MarkGame g;
    return mark_window_game(h, bt, o, &g, who) ? -1 : mark_coalitions_impl(h, bt, g, keep, n_coal, logits, stream, who);
}
extern "C" int cf_mark_window_shapley(cf_handle* h, const cf_batch* bt, const cf_mark_window_opts* o, float* phi, float* logits_all, void* stream) {
    const char* who = "cf_mark_window_shapley";
    MarkGame g;
    return mark_window_game(h, bt, o, &g, who, kCoalMaxS) ? -1 : mark_exact_impl(h, bt, g, kExactShapley, phi, logits_all, stream, who);
}
extern "C" int cf_mark_window_shapley_interactions(cf_handle* h, const cf_batch* bt, const cf_mark_window_opts* o, int index, float* inter, float* phi,
                                                   float* logits_all, void* stream) {
    const char* who = "cf_mark_window_shapley_interactions";
    MarkGame g;
    return mark_window_game(h, bt, o, &g, who, kCoalMaxS) ? -1
                                                          : mark_exact_impl(h, bt, g, kExactInteractions, inter, logits_all, stream, who, index, phi);
}
extern "C" int cf_mark_window_shapley_sampled(cf_handle* h, const cf_batch* bt, const cf_mark_window_opts* o, const uint8_t* perms, int n_perm,
                                              float* phi, float* se, float* logits_rows, void* stream) {
    const char* who = "cf_mark_window_shapley_sampled";
    MarkGame g;
    return mark_window_game(h, bt, o, &g, who) ? -1 : mark_sampled_impl(h, bt, g, perms, n_perm, phi, se, logits_rows, stream, who);
}

// the fine window game.
extern "C" int cf_mark_fine_coalitions(cf_handle* h, const cf_batch* bt, const cf_mark_fine_opts* o, const uint32_t* keep, int n_coal, float* logits,
                                       void* stream) {
    const char* who = "cf_mark_fine_coalitions";
    MarkGame g;
    return mark_fine_game(h, bt, o, &g, (hipStream_t)stream, who) ? -1 : mark_coalitions_impl(h, bt, g, keep, n_coal, logits, stream, who);
}
extern "C" int cf_mark_fine_shapley(cf_handle* h, const cf_batch* bt, const cf_mark_fine_opts* o, float* phi, float* logits_all, void* stream) {
    const char* who = "cf_mark_fine_shapley";
    MarkGame g;
    return mark_fine_game(h, bt, o, &g, (hipStream_t)stream, who, kCoalMaxS) ? -1 : mark_exact_impl(h, bt, g, kExactShapley, phi, logits_all, stream, who);
}
extern "C" int cf_mark_fine_shapley_interactions(cf_handle* h, const cf_batch* bt, const cf_mark_fine_opts* o, int index, float* inter, float* phi,
                                                 float* logits_all, void* stream) {
    const char* who = "cf_mark_fine_shapley_interactions";
    MarkGame g;
    return mark_fine_game(h, bt, o, &g, (hipStream_t)stream, who, kCoalMaxS)
               ? -1
               : mark_exact_impl(h, bt, g, kExactInteractions, inter, logits_all, stream, who, index, phi);
}
extern "C" int cf_mark_fine_shapley_sampled(cf_handle* h, const cf_batch* bt, const cf_mark_fine_opts* o, const uint8_t* perms, int n_perm, float* phi,
                                            float* se, float* logits_rows, void* stream) {
    const char* who = "cf_mark_fine_shapley_sampled";
    MarkGame g;
    return mark_fine_game(h, bt, o, &g, (hipStream_t)stream, who) ? -1 : mark_sampled_impl(h, bt, g, perms, n_perm, phi, se, logits_rows, stream, who);
}

// Sampled interaction indices of focal players, one entry point per wide kind.
extern "C" int cf_mark_shapley_interactions_sampled(cf_handle* h, const cf_batch* bt, const cf_mark_wide_opts* o, const uint8_t* perms, int n_perm,
                                                    const int* focal, int n_focal, int index, float* inter, float* se, float* phi, float* phi_se,
                                                    float* logits_rows, void* stream) {
    const char* who = "cf_mark_shapley_interactions_sampled";
    MarkGame g;
    return mark_wide_game(h, bt, o, &g, who)
               ? -1
               : mark_pairs_sampled_impl(h, bt, g, perms, n_perm, focal, n_focal, index, inter, se, phi, phi_se, logits_rows, stream, who);
}
extern "C" int cf_mark_window_shapley_interactions_sampled(cf_handle* h, const cf_batch* bt, const cf_mark_window_opts* o, const uint8_t* perms,
                                                           int n_perm, const int* focal, int n_focal, int index, float* inter, float* se, float* phi,
                                                           float* phi_se, float* logits_rows, void* stream) {
    const char* who = "cf_mark_window_shapley_interactions_sampled";
    MarkGame g;
    return mark_window_game(h, bt, o, &g, who)
               ? -1
               : mark_pairs_sampled_impl(h, bt, g, perms, n_perm, focal, n_focal, index, inter, se, phi, phi_se, logits_rows, stream, who);
}
extern "C" int cf_mark_fine_shapley_interactions_sampled(cf_handle* h, const cf_batch* bt, const cf_mark_fine_opts* o, const uint8_t* perms,
                                                         int n_perm, const int* focal, int n_focal, int index, float* inter, float* se, float* phi,
                                                         float* phi_se, float* logits_rows, void* stream) {
    const char* who = "cf_mark_fine_shapley_interactions_sampled";
    MarkGame g;
    return mark_fine_game(h, bt, o, &g, (hipStream_t)stream, who)
               ? -1
               : mark_pairs_sampled_impl(h, bt, g, perms, n_perm, focal, n_focal, index, inter, se, phi, phi_se, logits_rows, stream, who);
}
