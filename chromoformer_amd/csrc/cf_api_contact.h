// cf_api_contact.h -- host side of the contact games (cf_contact.h): cf_contact_coalitions, cf_contact_shapley, cf_contact_epistasis,
// cf_contact_shapley_interactions.  Part of cf_api.hip's single translation unit: included there behind cf_api_attrib.h, whose
// coalition_rows_by (the trunk once, k_pcre_stash, per chunk one expand launch and Regulation + head), word table, row buffer and
// exact-game reducers it uses; not on its own.
#pragma once

// What the four entry points check alike, in front of anything launched: the handle, the batch, the options.
static int contact_check(cf_handle* h, const cf_batch* bt, const cf_contact_opts* o, const char* who) {
    if (attrib_open(h, bt, false, who)) return -1;
    if (!o) return fail("%s: null opts", who);
    const int S = h->cfg.i_max;
    if (o->n_players < 1 || o->n_players > kCoalMaxS) return fail("%s: n_players = %d outside 1..%d", who, o->n_players, kCoalMaxS);
    if (!o->player_drop || !o->player_contact) return fail("%s: null player_drop / player_contact", who);
    for (int p = 0; p < o->n_players; ++p) {
        const unsigned d = o->player_drop[p], c = o->player_contact[p];
        if (!(d | c)) return fail("%s: player_drop[%d] = player_contact[%d] = 0: a player names at least one pCRE slot", who, p, p);
        if (d >> S) return fail("%s: player_drop[%d] = 0x%x names a pCRE slot >= i_max = %d", who, p, d, S);
        if (c >> S) return fail("%s: player_contact[%d] = 0x%x names a pCRE slot >= i_max = %d", who, p, c, S);
    }
    if (!std::isfinite(o->scale)) return fail("%s: scale = %g: a finite factor", who, (double)o->scale);
    return 0;
}

// The coalition words (validated) and the player words into the workspace's word table: [words | drop_p | contact_p].
static int contact_upload(cf_handle* h, const cf_contact_opts* o, const uint32_t* keep, int n_coal, hipStream_t st, const char* who) {
    const int P = o->n_players;
    if (n_coal < 1) return fail("%s: n_coal = %d: at least 1 coalition", who, n_coal);
    if (!keep) return fail("%s: null keep", who);
    for (int k = 0; P < 32 && k < n_coal; ++k)
        if (keep[k] >> P) return fail("%s: keep[%d] = 0x%x names a player >= n_players = %d", who, k, keep[k], P);
    if (attrib_ws(h, who) || h->aw.words.need((size_t)n_coal + 2 * P, 256, who)) return -1;
    unsigned* tab = h->aw.words;
    HIP_TRY(hipMemcpyAsync(tab, keep, (size_t)n_coal * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tab + n_coal, o->player_drop, P * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tab + n_coal + P, o->player_contact, P * sizeof(unsigned), hipMemcpyHostToDevice, st));
    return 0;
}

// The B * n_coal rows of the table contact_upload wrote: coalition_rows_by with k_contact_expand as the expand launch.
static int contact_rows(cf_handle* h, const cf_batch* bt, const cf_contact_opts* o, int n_coal, float* logits, hipStream_t st) {
    ContactExpandArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.players = h->aw.words + n_coal;
    ca.donor_freq = o->donor_freq;
    ca.scale = o->scale;
    ca.P = o->n_players;
    const int nres = h->cfg.n_res;
    return coalition_rows_by(h, bt, h->aw.words, n_coal, logits, st, [&](const CoalExpandArgs& ea, int n) {
        ca.c = ea;
        return launch_expand(k_contact_expand, "k_contact_expand", dim3(n, nres), kAblThreads, ca, st);
    });
}

extern "C" int cf_contact_coalitions(cf_handle* h, const cf_batch* bt, const cf_contact_opts* o, const uint32_t* keep, int n_coal, float* logits,
                                     void* stream) {
    const char* who = "cf_contact_coalitions";
    if (contact_check(h, bt, o, who)) return -1;
    if (!logits) return fail("%s: null logits", who);
    hipStream_t st = (hipStream_t)stream;
    if (contact_upload(h, o, keep, n_coal, st, who)) return -1;
    return contact_rows(h, bt, o, n_coal, logits, st);
}

// An exact game on the P players: all 2^P coalitions and k_shapley, the pair-deletion coalitions and k_epistasis, or all 2^P coalitions
// and k_shapley_pairs (with k_shapley if `phi` is given) -- all_words / pair_words and the reducers of cf_api_attrib.h.
enum ContactExact { kContactShapley, kContactEpistasis, kContactInteractions };
static int contact_exact(cf_handle* h, const cf_batch* bt, const cf_contact_opts* o, ContactExact what, float* out, float* logits_rows, void* stream,
                         const char* who, int index = 0, float* phi = nullptr) {
    if (contact_check(h, bt, o, who)) return -1;
    const int P = o->n_players;
    if (what == kContactInteractions) {
        if (interactions_check(index, P, out, who)) return -1;
    } else if (!out) {
        return fail(what == kContactEpistasis ? "%s: null eps" : "%s: null phi", who);
    } else if (what == kContactEpistasis && P < 2) {
        return fail("%s: %d player: a pair needs at least 2", who, P);
    }
    const std::vector<uint32_t> keep = what == kContactEpistasis ? pair_words(P) : all_words(P);
    const int R = (int)keep.size();
    float* rows = coalition_out_rows(h, logits_rows, R, who);
    if (!rows) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (contact_upload(h, o, keep.data(), R, st, who) || contact_rows(h, bt, o, R, rows, st)) return -1;
    if (what == kContactInteractions) return launch_interactions(h, bt->B, P, index, rows, out, phi, st);
    return what == kContactEpistasis ? launch_epistasis(h, bt->B, P, rows, out, st) : launch_shapley(h, bt->B, P, rows, out, st);
}

extern "C" int cf_contact_shapley(cf_handle* h, const cf_batch* bt, const cf_contact_opts* o, float* phi, float* logits_all, void* stream) {
    return contact_exact(h, bt, o, kContactShapley, phi, logits_all, stream, "cf_contact_shapley");
}

extern "C" int cf_contact_epistasis(cf_handle* h, const cf_batch* bt, const cf_contact_opts* o, float* eps, float* logits_pairs, void* stream) {
    return contact_exact(h, bt, o, kContactEpistasis, eps, logits_pairs, stream, "cf_contact_epistasis");
}

extern "C" int cf_contact_shapley_interactions(cf_handle* h, const cf_batch* bt, const cf_contact_opts* o, int index, float* inter, float* phi,
                                               float* logits_all, void* stream) {
    return contact_exact(h, bt, o, kContactInteractions, inter, logits_all, stream, "cf_contact_shapley_interactions", index, phi);
}
