// TEST-ONLY: the generating calls (ftz_generate_transfers / ftz_generate_issues)
// on the CPU.  The generating plans (host/planner_prove.cpp plan_gen_*) run
// through the existing executor of emu_exec.cpp -- with the jobs of the new
// emission level held back, which that executor does not know -- and then the
// two k_b64 launches of the device path run here over the arena it left:
// level 0 (inner documents into the outer proof in the arena, owners and issuer
// into the action and metadata documents), level 1 (the outer proof into the
// action, the documents and commitments into the output).  The results are
// split as runtime.hip gen_collect splits them.
#include "emu_exec.cpp"

namespace {

struct Orders {
  std::vector<GenTransfer> t;
  std::vector<GenIssue> is;
  std::vector<uint8_t> vals;
  std::vector<uint32_t> n_out;
  size_t tokens = 0;
};

void be32_u64(uint8_t* b, uint64_t v) {
  memset(b, 0, 32);
  for (int q = 0; q < 8; q++) b[31 - q] = (uint8_t)(v >> (8 * q));
}
const GenBytes* as_gen(const ftz_bytes* b) { return reinterpret_cast<const GenBytes*>(b); }

void to_orders(size_t n, const ftz_transfer_order* o, Orders& g) {
  for (size_t i = 0; i < n; i++) g.tokens += o[i].n_out;
  g.vals.resize(32 * g.tokens + 32);
  g.t.resize(n);
  g.n_out.resize(n);
  size_t t = 0;
  for (size_t i = 0; i < n; i++) {
    for (uint32_t k = 0; k < o[i].n_out; k++) be32_u64(&g.vals[32 * (t + k)], o[i].out_values[k]);
    g.t[i].w = {o[i].inputs, o[i].n_in,  nullptr,   o[i].n_out,    o[i].in_values, o[i].in_bfs, &g.vals[32 * t],
                nullptr,     o[i].type, o[i].type_len, o[i].seed};
    g.t[i].ids = as_gen(o[i].input_ids);
    g.t[i].owners = as_gen(o[i].out_owners);
    g.n_out[i] = o[i].n_out;
    t += o[i].n_out;
  }
}
void to_orders(size_t n, const ftz_issue_order* o, Orders& g) {
  for (size_t i = 0; i < n; i++) g.tokens += o[i].n_out;
  g.vals.resize(32 * g.tokens + 32);
  g.is.resize(n);
  g.n_out.resize(n);
  size_t t = 0;
  for (size_t i = 0; i < n; i++) {
    for (uint32_t k = 0; k < o[i].n_out; k++) be32_u64(&g.vals[32 * (t + k)], o[i].values[k]);
    g.is[i].w = {nullptr, o[i].n_out, &g.vals[32 * t], nullptr, o[i].type, o[i].type_len, 0, o[i].seed};
    g.is[i].issuer = {o[i].issuer.p, o[i].issuer.len};
    g.is[i].owners = as_gen(o[i].owners);
    g.n_out[i] = o[i].n_out;
    t += o[i].n_out;
  }
}

template <class G>
std::string totals(const PPInfo& pp, size_t n, const G* g, size_t* act, size_t* meta) {
  GenSizeCache* cache = gen_size_cache_new();
  std::vector<uint32_t> len;
  std::string e;
  *act = *meta = 0;
  for (size_t i = 0; i < n && e.empty(); i++) {
    len.assign((size_t)g[i].w.n_out + 1, 0);
    e = gen_sizes(pp, g[i], i, cache, len.data());
    *act += len[0];
    for (size_t k = 1; k < len.size(); k++) *meta += len[k];
  }
  gen_size_cache_free(cache);
  return e;
}

// the new emission level over the arena the executor left (k_b64 level 0 / 1)
void run_level(const std::vector<B64Job>& jobs, uint32_t level, uint8_t* arena, uint8_t* out) {
  for (const B64Job& j : jobs) {
    if (((j.len & B64_L2) != 0) != (level != 0)) continue;
    for (uint32_t u = 0; u < job_b64_units(j); u++) job_b64_unit(j, u, arena, out);
  }
}

struct Sink {
  uint8_t *act, *meta, *coms;
  size_t *act_off, *meta_off;
  int32_t* codes;
};

std::string plan_gen(const PPInfo& pp, size_t n, const GenTransfer* g, Plan& p) {
  return plan_gen_transfers(pp, n, g, p, 4);
}
std::string plan_gen(const PPInfo& pp, size_t n, const GenIssue* g, Plan& p) { return plan_gen_issues(pp, n, g, p, 4); }

// returns 0, -1 (refused, message in err) or -2 (capacity, the needed sizes in err)
template <class G>
long generate(EmuCtx* c, size_t n, const G* g, const Orders& o, size_t act_cap, size_t meta_cap, const Sink& s,
              char* err, size_t errlen) {
  size_t need_a = 0, need_m = 0;
  std::string e = totals(c->pp, n, g, &need_a, &need_m);
  if (!e.empty()) {
    snprintf(err, errlen, "%s", e.c_str());
    return -1;
  }
  if (need_a > act_cap || need_m > meta_cap) {
    snprintf(err, errlen, "generate: buffers too small: need %zu action bytes and %zu metadata bytes", need_a, need_m);
    return -2;
  }
  s.act_off[0] = s.meta_off[0] = 0;
  if (n == 0) return 0;
  emu_ensure_sig_tables(c);
  Plan p;
  e = plan_gen(c->pp, n, g, p);
  if (!e.empty()) {
    snprintf(err, errlen, "%s", e.c_str());
    return -1;
  }
  // hold the new level's jobs back from the existing executor
  std::vector<B64Job> held;
  held.swap(p.b64);
  std::vector<uint8_t> proofs(p.out.size() + 1);  // what the executor takes for proofs: the output images
  std::vector<size_t> offs(n + 1);
  std::vector<int32_t> codes(n);
  long r = run_prove_plan(c, p, n, proofs.data(), proofs.size(), offs.data(), codes.data());
  if (r < 0) {
    snprintf(err, errlen, "executor refused the plan");
    return -1;
  }
  // p.out holds the images the copy jobs wrote; the arena everything up to k_emit
  run_level(held, 0, p.arena.data(), p.out.data());
  run_level(held, 1, p.arena.data(), p.out.data());
  size_t act_w = 0, meta_w = 0, tok = 0, q = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t no = o.n_out[i];
    const uint8_t* blk = p.out.data() + p.out_off[i];
    const uint32_t* len = p.gen_len.data() + q;
    q += 1 + no;
    s.codes[i] = codes[i];
    s.act_off[i] = act_w;
    size_t at = len[0];
    if (codes[i] == 0) {
      memcpy(s.act + act_w, blk, len[0]);
      act_w += len[0];
    }
    for (uint32_t k = 0; k < no; k++) {
      s.meta_off[tok + k] = meta_w;
      if (codes[i] == 0) {
        memcpy(s.meta + meta_w, blk + at, len[1 + k]);
        meta_w += len[1 + k];
      }
      at += len[1 + k];
    }
    if (s.coms) {
      if (codes[i] == 0)
        memcpy(s.coms + 64 * tok, blk + at, 64 * (size_t)no);
      else
        memset(s.coms + 64 * tok, 0, 64 * (size_t)no);
    }
    tok += no;
  }
  s.act_off[n] = act_w;
  s.meta_off[tok] = meta_w;
  return 0;
}

}  // namespace

extern "C" {

long gen_emu_transfers(void* ctx, size_t n, const ftz_transfer_order* o, uint8_t* act, size_t act_cap, size_t* act_off,
                       uint8_t* meta, size_t meta_cap, size_t* meta_off, uint8_t* coms, int32_t* codes, char* err,
                       size_t errlen) {
  Orders g;
  to_orders(n, o, g);
  return generate((EmuCtx*)ctx, n, g.t.data(), g, act_cap, meta_cap, Sink{act, meta, coms, act_off, meta_off, codes},
                  err, errlen);
}

long gen_emu_issues(void* ctx, size_t n, const ftz_issue_order* o, uint8_t* act, size_t act_cap, size_t* act_off,
                    uint8_t* meta, size_t meta_cap, size_t* meta_off, uint8_t* coms, int32_t* codes, char* err,
                    size_t errlen) {
  Orders g;
  to_orders(n, o, g);
  return generate((EmuCtx*)ctx, n, g.is.data(), g, act_cap, meta_cap, Sink{act, meta, coms, act_off, meta_off, codes},
                  err, errlen);
}

long gen_emu_transfers_size(void* ctx, size_t n, const ftz_transfer_order* o, size_t* act, size_t* meta, char* err,
                            size_t errlen) {
  Orders g;
  to_orders(n, o, g);
  std::string e = totals(((EmuCtx*)ctx)->pp, n, g.t.data(), act, meta);
  snprintf(err, errlen, "%s", e.c_str());
  return e.empty() ? 0 : -1;
}

long gen_emu_issues_size(void* ctx, size_t n, const ftz_issue_order* o, size_t* act, size_t* meta, char* err,
                         size_t errlen) {
  Orders g;
  to_orders(n, o, g);
  std::string e = totals(((EmuCtx*)ctx)->pp, n, g.is.data(), act, meta);
  snprintf(err, errlen, "%s", e.c_str());
  return e.empty() ? 0 : -1;
}

// ftz_token_request_encode (runtime.hip) over the same encoder
long gen_emu_encode_request(const ftz_bytes* const lists[4], const size_t counts[4], uint8_t* out, size_t cap) {
  const GenBytes* l[4];
  for (int f = 0; f < 4; f++) l[f] = as_gen(lists[f]);
  size_t need = der_encode_token_request(l, counts, nullptr);
  if (out && cap >= need) der_encode_token_request(l, counts, out);
  return (long)need;
}

// ftz_token_request_decode (request_rt.hip) over the same decoder: 0 or -1
long gen_emu_decode_request(const uint8_t* raw, size_t len, size_t counts[4], ftz_bytes* elems, size_t cap) {
  std::vector<Slice> f[4];
  if (!der_token_request(raw, len, f).empty()) return -1;
  size_t o = 0;
  for (int k = 0; k < 4; k++) {
    counts[k] = f[k].size();
    for (const Slice& s : f[k])
      if (o < cap) elems[o++] = ftz_bytes{s.p, s.len};
  }
  return 0;
}

}  // extern "C"
