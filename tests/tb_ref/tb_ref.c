/* TEST INFRASTRUCTURE: independent endgame-table generator and certificate checker, the yardstick for the product's
 * tablebases (matrix0_amd/csrc/tb_core.h).  Plain C on the ORACLE's rules engine (oracle/chess_oracle.c: 8x8 mailbox,
 * make-and-test legality -- not the product's bitboards) and with a different loop: the successors of every entry are
 * listed once, then whole-table passes over a snapshot of the previous pass run until nothing changes and nothing is
 * pending; pass k assigns exactly the entries whose depth works out as k.
 *
 * THE CONTRACT shared with the product (restated, not included):
 *   Signature  "K<white men>K<black men>", men ordered Q > R > B > N > P; the greater side is written first and is White
 *              in the table; sides compare by number of men, then lexicographically in that order.  A position whose
 *              Black side is greater is looked up through its colour flip (square ^ 56, colours and side to move swapped);
 *              equal material is not flipped.  KPKP and anything above four men is out of scope.
 *   Men order  White king, White's other men as written, Black king, Black's other men; identical men of a side in
 *              ascending square order (a1 = 0 ... h8 = 63).
 *   Index      stm * 64^n + sum(square_i * 64^i); stm = 0 White to move, 1 Black to move; 2 * 64^n entries.
 *   Entry      one byte: 0 draw; 255 invalid (two men on a square, identical men out of order, pawn on rank 1 or 8,
 *              adjacent kings, the side not to move in check); 1 + d decided in d plies, d even = side to move is mated
 *              in d (0: checkmated), d odd = side to move mates in d.  No 50-move rule, castling or en passant.
 *
 *   tb_ref gen  <dir> SIG...               generate SIG... in the given order (dependencies first) into <dir>/<SIG>.bin
 *   tb_ref cert <dir> SIG <seed> <samples>  check the certificate of <dir>/SIG.bin on <samples> entries drawn with <seed>
 *                                           plus every entry with d <= 2; the tables its moves lead into are read from <dir>
 */
#include "../../oracle/chess_oracle.c"

typedef struct {
    char name[8];
    int n, nw, nb;
    int wt[2], bt[2];          /* oracle piece types: 1..5 = P N B R Q */
    uint8_t* bytes;
    size_t size;
} Table;

static Table g_tab[64];
static int g_ntab;
static const char* g_dir = ".";

static int type_of_letter(char c) {
    const char* L = "PNBRQ";
    const char* q = strchr(L, c);
    return (q && c) ? (int)(q - L) + 1 : 0;
}

static int parse_name(const char* name, Table* t) {
    const char* c = name;
    memset(t, 0, sizeof(*t));
    if (strlen(name) > 6 || *c != 'K') return -1;
    for (++c; *c && *c != 'K'; ++c) { if (t->nw >= 2 || !type_of_letter(*c)) return -1; t->wt[t->nw++] = type_of_letter(*c); }
    if (*c != 'K') return -1;
    for (++c; *c; ++c) { if (t->nb >= 2 || !type_of_letter(*c)) return -1; t->bt[t->nb++] = type_of_letter(*c); }
    t->n = 2 + t->nw + t->nb;
    if (t->n > 4) return -1;
    strcpy(t->name, name);
    t->size = (size_t)2 << (6 * t->n);
    return 0;
}

static Table* find_table(const char* name) {
    int i;
    for (i = 0; i < g_ntab; ++i) if (!strcmp(g_tab[i].name, name)) return &g_tab[i];
    return NULL;
}

static Table* load_table(const char* name) {
    Table* t = find_table(name);
    char path[1024];
    FILE* f;
    if (t) return t->bytes ? t : NULL;
    t = &g_tab[g_ntab];
    if (g_ntab >= 63 || parse_name(name, t)) return NULL;
    g_ntab++;                                            /* remembered even when the file is missing */
    snprintf(path, sizeof(path), "%s/%s.bin", g_dir, name);
    f = fopen(path, "rb");
    if (!f) return NULL;
    t->bytes = (uint8_t*)malloc(t->size);
    if (fread(t->bytes, 1, t->size, f) != t->size || fgetc(f) != EOF) { free(t->bytes); t->bytes = NULL; }
    fclose(f);
    return t->bytes ? t : NULL;
}

/* ---- position -> (signature, index) ---- */
typedef struct { int cnt; int king; int type[2]; int sq[2]; } Side;

static int collect(const OPos* p, int white, Side* s) {
    int sq, i;
    s->cnt = 0; s->king = -1;
    for (sq = 0; sq < 64; ++sq) {                        /* ascending squares: identical men come out in index order */
        int pc = p->sq[sq];
        if (!pc || (IS_WHITE(pc) != 0) != (white != 0)) continue;
        if (PT(pc) == 6) { if (s->king >= 0) return -1; s->king = sq; continue; }
        if (s->cnt >= 2) return -1;
        s->type[s->cnt] = PT(pc); s->sq[s->cnt] = sq; s->cnt++;
    }
    if (s->king < 0) return -1;
    if (s->cnt == 2 && s->type[1] > s->type[0]) {        /* stronger man first; equal types keep their square order */
        i = s->type[0]; s->type[0] = s->type[1]; s->type[1] = i;
        i = s->sq[0]; s->sq[0] = s->sq[1]; s->sq[1] = i;
    }
    return 0;
}

static int side_greater(const Side* a, const Side* b) {   /* a > b */
    int i;
    if (a->cnt != b->cnt) return a->cnt > b->cnt;
    for (i = 0; i < a->cnt; ++i) if (a->type[i] != b->type[i]) return a->type[i] > b->type[i];
    return 0;
}

/* 0 and name/idx, or -1 when the position is outside any table's domain (more than 4 men, 3 men beside a king) */
static int locate(const OPos* pin, char* name, size_t* idx) {
    OPos p = *pin;
    Side w, b;
    int i, k = 0, sh = 0;
    size_t x = 0;
    const char* L = " PNBRQ";
    if (collect(&p, 1, &w) || collect(&p, 0, &b) || w.cnt + b.cnt > 2) return -1;
    if (side_greater(&b, &w)) {                          /* the colour flip, done on the board itself */
        OPos q;
        memset(&q, 0, sizeof(q));
        for (i = 0; i < 64; ++i) {
            int pc = pin->sq[i];
            if (pc) q.sq[i ^ 56] = (int8_t)(IS_WHITE(pc) ? pc + 6 : pc - 6);
        }
        q.turn = (int8_t)!pin->turn; q.ep = -1; q.fullmove = 1;
        p = q;
        if (collect(&p, 1, &w) || collect(&p, 0, &b)) return -1;
    }
    name[k++] = 'K';
    for (i = 0; i < w.cnt; ++i) name[k++] = L[w.type[i]];
    name[k++] = 'K';
    for (i = 0; i < b.cnt; ++i) name[k++] = L[b.type[i]];
    name[k] = 0;
    x |= (size_t)w.king << sh; sh += 6;
    for (i = 0; i < w.cnt; ++i) { x |= (size_t)w.sq[i] << sh; sh += 6; }
    x |= (size_t)b.king << sh; sh += 6;
    for (i = 0; i < b.cnt; ++i) { x |= (size_t)b.sq[i] << sh; sh += 6; }
    x |= (size_t)(p.turn ? 0 : 1) << sh;
    *idx = x;
    return 0;
}

/* ---- index -> position; 0 = a legal placement, -1 = an invalid entry ---- */
static int decode(const Table* t, size_t idx, OPos* p) {
    int sq[4] = {0, 0, 0, 0}, i, wk, bk, dr, df;
    memset(p, 0, sizeof(*p));
    p->ep = -1; p->fullmove = 1;
    for (i = 0; i < t->n; ++i) sq[i] = (int)((idx >> (6 * i)) & 63);
    p->turn = (int8_t)(((idx >> (6 * t->n)) & 1) ? 0 : 1);
    wk = sq[0]; bk = sq[1 + t->nw];
    for (i = 0; i < t->n; ++i) {
        int white = i <= t->nw, j = white ? i - 1 : i - t->nw - 2;
        int type = j < 0 ? 6 : (white ? t->wt[j] : t->bt[j]);
        if (p->sq[sq[i]]) return -1;
        if (type == 1 && (rank_of(sq[i]) == 0 || rank_of(sq[i]) == 7)) return -1;
        if (j == 1 && (white ? t->wt[0] == t->wt[1] : t->bt[0] == t->bt[1]) && sq[i - 1] > sq[i]) return -1;
        p->sq[sq[i]] = (int8_t)((white ? 0 : 6) + type);
    }
    dr = rank_of(wk) - rank_of(bk); df = file_of(wk) - file_of(bk);
    if (dr >= -1 && dr <= 1 && df >= -1 && df <= 1) return -1;
    {   /* the side that has just moved must not be in check */
        OPos q = *p;
        q.turn = (int8_t)!p->turn;
        if (o_in_check(&q)) return -1;
    }
    return 0;
}

/* ---- generation ---- */
#define INF 1000

static int generate(const char* name) {
    Table* t = find_table(name);
    size_t e, nsucc = 0, cap = 0;
    uint32_t *succ = NULL, *start;
    int16_t *sub_min_lost, *sub_max_won;
    uint8_t *sub_not_won, *open, *snap;
    int pass, changed, pending, maxd = -1;
    if (t) return t->bytes ? 0 : -1;
    t = &g_tab[g_ntab];
    if (g_ntab >= 63 || parse_name(name, t)) { fprintf(stderr, "bad signature %s\n", name); return -1; }
    g_ntab++;
    t->bytes = (uint8_t*)calloc(t->size, 1);
    snap = (uint8_t*)malloc(t->size);
    start = (uint32_t*)calloc(t->size + 1, sizeof(uint32_t));
    sub_min_lost = (int16_t*)malloc(t->size * sizeof(int16_t));
    sub_max_won = (int16_t*)malloc(t->size * sizeof(int16_t));
    sub_not_won = (uint8_t*)calloc(t->size, 1);
    open = (uint8_t*)calloc(t->size, 1);
    /* pass 0: placements, mates, stalemates; the successors of everything else, those in finished tables folded at once */
    for (e = 0; e < t->size; ++e) {
        OPos p;
        OMove mv[MAX_MOVES];
        int nm, i;
        start[e] = (uint32_t)nsucc;
        sub_min_lost[e] = INF; sub_max_won[e] = -1;
        if (decode(t, e, &p)) { t->bytes[e] = 255; continue; }
        nm = o_gen_legal(&p, mv);
        if (nm == 0) { t->bytes[e] = o_in_check(&p) ? 1 : 0; if (t->bytes[e]) maxd = maxd < 0 ? 0 : maxd; continue; }
        open[e] = 1;
        for (i = 0; i < nm; ++i) {
            OPos q = p;
            char sname[8];
            size_t sidx;
            o_make(&q, mv[i]);
            if (locate(&q, sname, &sidx)) { fprintf(stderr, "%s: successor outside every table\n", name); return -1; }
            if (!strcmp(sname, name)) {
                if (nsucc == cap) { cap = cap ? cap * 2 : 1 << 20; succ = (uint32_t*)realloc(succ, cap * sizeof(uint32_t)); }
                succ[nsucc++] = (uint32_t)sidx;
            } else {
                Table* s = find_table(sname);
                int v, d;
                if (!s || !s->bytes) { fprintf(stderr, "%s needs %s first\n", name, sname); return -1; }
                v = s->bytes[sidx];
                if (v == 255) { fprintf(stderr, "%s: a legal move reaches an invalid entry of %s\n", name, sname); return -1; }
                d = v - 1;
                if (v == 0) sub_not_won[e] = 1;
                else if (d % 2 == 0) { sub_not_won[e] = 1; if (d < sub_min_lost[e]) sub_min_lost[e] = (int16_t)d; }
                else if (d > sub_max_won[e]) sub_max_won[e] = (int16_t)d;
            }
        }
    }
    start[t->size] = (uint32_t)nsucc;
    for (pass = 1;; ++pass) {
        if (pass > 253) { fprintf(stderr, "%s: depth does not fit a byte\n", name); return -1; }
        memcpy(snap, t->bytes, t->size);
        changed = 0; pending = 0;
        for (e = 0; e < t->size; ++e) {
            int min_lost, max_won, not_won, depth = -1;
            uint32_t k;
            if (!open[e]) continue;
            min_lost = sub_min_lost[e]; max_won = sub_max_won[e]; not_won = sub_not_won[e];
            for (k = start[e]; k < start[e + 1]; ++k) {
                int v = snap[succ[k]], d = v - 1;
                if (v == 0) not_won = 1;
                else if (d % 2 == 0) { not_won = 1; if (d < min_lost) min_lost = d; }
                else if (d > max_won) max_won = d;
            }
            if (min_lost < INF) depth = min_lost + 1;          /* a move into a lost position: win, as fast as known so far */
            else if (!not_won) depth = max_won + 1;            /* every move into a won position: loss, as slow as possible */
            if (depth < 0) continue;
            if (depth < pass) { fprintf(stderr, "%s: entry %zu has depth %d in pass %d\n", name, e, depth, pass); return -1; }
            if (depth > pass) { pending = 1; continue; }       /* its turn comes in pass `depth` (a faster win may show up) */
            t->bytes[e] = (uint8_t)(1 + depth); open[e] = 0; changed++; maxd = depth;
        }
        if (!changed && !pending) break;
    }
    printf("%s largest_d %d passes %d\n", name, maxd, pass);
    free(snap); free(start); free(succ); free(sub_min_lost); free(sub_max_won); free(sub_not_won); free(open);
    return 0;
}

/* ---- certificate ---- */
static long g_checked, g_viol, g_skipped;

static void violation(const Table* t, size_t e, const char* what) {
    if (g_viol < 20) fprintf(stderr, "%s[%zu] = %d: %s\n", t->name, e, t->bytes[e], what);
    g_viol++;
}

static void check_entry(const Table* t, size_t e) {
    OPos p;
    OMove mv[MAX_MOVES];
    int v = t->bytes[e], nm, i, d = v - 1;
    int min_lost = INF, max_won = -1, any_draw = 0, any_not_won = 0;
    g_checked++;
    if (decode(t, e, &p)) { if (v != 255) violation(t, e, "an illegal placement is not marked invalid"); return; }
    if (v == 255) { violation(t, e, "a legal placement is marked invalid"); return; }
    nm = o_gen_legal(&p, mv);
    if (nm == 0) {
        if (o_in_check(&p) ? v != 1 : v != 0) violation(t, e, "checkmate must be 1 and stalemate 0");
        return;
    }
    if (v == 1) { violation(t, e, "d = 0 but the side to move has a legal move"); return; }
    for (i = 0; i < nm; ++i) {
        OPos q = p;
        char sname[8];
        size_t sidx;
        Table* s;
        int sv;
        o_make(&q, mv[i]);
        if (locate(&q, sname, &sidx) || !(s = load_table(sname))) { g_skipped++; return; }
        sv = s->bytes[sidx];
        if (sv == 255) { violation(t, e, "a legal move reaches an invalid entry"); return; }
        if (sv == 0) { any_draw = 1; any_not_won = 1; }
        else if ((sv - 1) % 2 == 0) { any_not_won = 1; if (sv - 1 < min_lost) min_lost = sv - 1; }
        else if (sv - 1 > max_won) max_won = sv - 1;
    }
    if (v == 0) {
        if (min_lost < INF) violation(t, e, "a draw with a move into a lost position");
        else if (!any_draw) violation(t, e, "a draw without a move into a draw");
    } else if (d % 2 == 1) {
        if (min_lost != d - 1) violation(t, e, "a win in d needs a lost successor with d - 1 and none smaller");
    } else {
        if (any_not_won || max_won != d - 1) violation(t, e, "a loss in d needs only won successors, the largest d - 1");
    }
}

static uint64_t splitmix(uint64_t* s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    int i;
    if (argc >= 4 && !strcmp(argv[1], "gen")) {
        g_dir = argv[2];
        for (i = 3; i < argc; ++i) {
            char path[1024];
            FILE* f;
            Table* t;
            if (generate(argv[i])) return 1;
            t = find_table(argv[i]);
            snprintf(path, sizeof(path), "%s/%s.bin", g_dir, argv[i]);
            f = fopen(path, "wb");
            if (!f || fwrite(t->bytes, 1, t->size, f) != t->size || fclose(f)) { fprintf(stderr, "cannot write %s\n", path); return 1; }
        }
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "cert")) {
        Table* t;
        uint64_t seed = strtoull(argv[4], NULL, 10);
        long samples = atol(argv[5]), k, low = 0;
        size_t e;
        g_dir = argv[2];
        t = load_table(argv[3]);
        if (!t) { fprintf(stderr, "cannot read table %s from %s\n", argv[3], g_dir); return 1; }
        for (k = 0; k < samples; ++k) check_entry(t, (size_t)(splitmix(&seed) % t->size));
        for (e = 0; e < t->size; ++e)
            if (t->bytes[e] >= 1 && t->bytes[e] <= 3) { check_entry(t, e); low++; }
        printf("%s checked %ld sampled %ld low_d %ld violations %ld skipped %ld\n", t->name, g_checked, samples, low, g_viol, g_skipped);
        return (g_viol || g_skipped) ? 2 : 0;
    }
    fprintf(stderr, "usage: tb_ref gen <dir> SIG... | tb_ref cert <dir> SIG <seed> <samples>\n");
    return 1;
}
