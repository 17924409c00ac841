/* ftsamd -- MI355X batch verifier for the zkatdlog (nogh) driver of the
 * Fabric Token SDK.  C ABI: plain pointers and sizes, no torch / HIP types.
 *
 * Reference interfaces this boundary replaces (paths relative to
 * /root/reference/token/core/zkatdlog/):
 *   ftz_ctx_create        crypto/setup.go:134-151   PublicParams.Deserialize (+ Validate :238-273)
 *                         nogh/driver/driver.go:114-124 Driver.NewValidator (PP parsed once per process)
 *   ftz_verify_transfers  crypto/transfer/transfer.go:66-77,124-154
 *                         transfer.NewVerifier(inputs, outputs, pp).Verify(proof)
 *                         as called by crypto/validator/validator_transfer.go:84-98
 *                         TransferZKProofValidate (inputs = ledger commitments)
 *   ftz_verify_issues     crypto/issue/issue.go:194-223
 *                         issue.NewVerifier(tokens, anonymous, pp).Verify(proof)
 *                         as called by crypto/validator/validator.go:181-191 verifyIssue
 * The Go error classes map to the FTZ_ERR_* codes below; a proof on which the
 * reference would panic (nil dereference, foreign curve id) is reported as
 * FTZ_ERR_PANIC (reject) instead of crashing the process.
 *
 * Thread-safety and batching: a context may be used from any number of
 * threads.  ftz_verify_transfers / ftz_verify_issues are synchronous for the
 * caller but go through one job engine per context: a call of any size is cut
 * into device batches of at most `batch` proofs (planned on host threads while
 * earlier batches run on the GPU, `slots` batches in flight), and concurrent
 * small calls -- the Go shim verifies one TransferAction per call
 * (validator_transfer.go:84-98) -- are coalesced into shared batches
 * (micro-batching).  Results are delivered per call.
 */
#ifndef FTSAMD_H
#define FTSAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-proof verdict codes (0 = accept) */
#define FTZ_OK 0
#define FTZ_ERR_PARSE 1      /* json / base64 / element decoding failed            */
#define FTZ_ERR_MALFORMED 2  /* "not well formed", nil fields, length mismatches    */
#define FTZ_ERR_WF 3         /* "invalid zero-knowledge transfer" / issue WF        */
#define FTZ_ERR_RANGE 4      /* "invalid range proof"                               */
#define FTZ_ERR_MEMBERSHIP 5 /* "invalid membership proof"                          */
#define FTZ_ERR_PANIC 6      /* the reference would panic on this proof             */
#define FTZ_ERR_OPENING 7    /* audit: "output ... does not match the provided opening" */
/* 8 = FTZ_ERR_INPUT (token requests, below) */

/* API return codes */
#define FTZ_SUCCESS 0
#define FTZ_E_INVALID (-1) /* bad argument                                         */
#define FTZ_E_PP (-2)      /* public parameters rejected                            */
#define FTZ_E_DEVICE (-3)  /* no usable MI355X / HIP error (see ftz_last_error)     */
#define FTZ_E_NOMEM (-4)

typedef struct ftz_ctx ftz_ctx;
typedef struct ftz_batch ftz_batch;

/* One transfer action: commitments are 64-byte gnark G1 RawBytes (X||Y). */
typedef struct {
  const uint8_t* inputs; /* n_in  x 64 bytes: input token commitments (ledger)   */
  uint32_t n_in;
  const uint8_t* outputs; /* n_out x 64 bytes: output token commitments          */
  uint32_t n_out;
  const uint8_t* proof; /* json(transfer.Proof) as carried in TransferAction.Proof */
  size_t proof_len;
} ftz_transfer;

typedef struct {
  const uint8_t* outputs; /* n_out x 64 bytes: issued token commitments          */
  uint32_t n_out;
  const uint8_t* proof; /* json(issue.Proof)                                      */
  size_t proof_len;
  uint8_t anonymous; /* IssueAction.Anonymous                                     */
} ftz_issue;

/* Per-kernel timing of the last ftz_batch_run (HIP events on the batch stream). */
#define FTZ_NKERNELS 12
typedef struct {
  /* decode, zr, hash_pre, scalar, g1_pairing, g2 + pair-2 lines (stream 3), miller, fexp, g1_side (stream 2), hash,
   * verdict, total */
  float ms[FTZ_NKERNELS];
  uint64_t jobs[FTZ_NKERNELS];
} ftz_stats;

/* Final exponentiation variant [EXT] (GT bytes feed every
 * membership transcript, sigproof/membership.go:247,260-277):
 *   FTZ_FEXP_EXACT    f^((p^12-1)/r) -- the Scott et al. (ePrint 2008/490) hard
 *                     part of gnark-crypto v0.6.0 (go.mod:53), the default;
 *   FTZ_FEXP_FUENTES  f^(2x(6x^2+3x+1)(p^12-1)/r) -- the Fuentes-Castaneda et al.
 *                     chain later gnark-crypto releases use. */
#define FTZ_FEXP_EXACT 0
#define FTZ_FEXP_FUENTES 1

typedef struct {
  uint32_t struct_size; /* sizeof(ftz_options)                                          */
  uint32_t batch;       /* max proofs per device batch (default 8192: 4096 leaves the
                           pairing kernels at 1.6 sextet waves per SIMD, profiles/r02g_*) */
  uint32_t slots;       /* passes the job engine runs side by side, each on a stream triple
                           of its own (default 4; DESIGN section 2: 1 / 2 / 3 / 4 / 5
                           batches in flight gave 400k / 444k / 500k / 538k / 542k
                           transfers/s).  The context has min(slots, 4) triples; slots
                           beyond 4 share them (and count as the next multiple of 4).
                           The engine owns one buffer set per slot, and `lookahead`
                           more per triple                                          */
  uint32_t window_us;   /* micro-batching: how long a partial batch may wait for more
                           callers while the GPU is busy (default 1000; seam sweep,
                           profiles/r03k/seamsweep.jsonl)                                */
  uint32_t threads;     /* host planning threads (0: min(16, hardware threads))         */
  uint32_t fexp;        /* FTZ_FEXP_EXACT (default) or FTZ_FEXP_FUENTES                 */
  uint32_t hold_inflight; /* a partial batch waits (up to window_us) for more callers
                           only while at least this many batches are in flight
                           (default 2; 0: always, also with the GPU idle -- closed-loop
                           callers resubmit together; FTZ_HOLD_NEVER: ship at once)       */
  uint32_t small_pass;  /* device passes of at most this many G2 jobs run the low-latency
                           layout of the t' / pair-2 line stage (six lanes per job
                           instead of one; same bytes); default 4096, 0 = never; an
                           explicit ftz_ctx_set_layout(FTZ_STAGE_G2LINES) overrides it  */
  uint32_t msm_window_bits; /* MSM planner overrides (ftz_msm_*), 0 = the planner's choice: */
  uint32_t msm_slot_cap;    /*   window bits c, bucket slot cap T, slots per segment S    */
  uint32_t msm_seg_slots;
  uint32_t msm_glv;     /* 1 (default): GLV-split scalars in the MSM; 0: plain 256-bit   */
  uint32_t msm_precompute; /* 1: resident-point MSM -- ftz_msm_load also stores 2^(c w) P
                           for every window w (W x the point memory) and runs use one shared
                           bucket set and no Horner chain; for fixed bases (ftz_msm_set_scalars)
                           0 (default): plain variable-base Pippenger                      */
  uint32_t prover_tables; /* 1 (default): the first ftz_prove_* call builds fixed-base tables
                           of the PP's digit signatures R_d, S_d (32 MB per point with
                           16-bit windows: 2 x base x 32 MB, 6.4 GB at base 100, once per
                           context) and proves through them and fixed-G2 pairings; if
                           that allocation fails the context proves on the
                           variable-base path instead (same bytes, slower) and does not
                           retry.  0: never build them (variable-base path).            */
  uint32_t msm_radix_bits; /* MSM sort digit bits per radix pass: 0 = the planner's choice
                           (9 where it saves a pass, else 8), or 8 / 9                   */
  uint32_t first_pass;  /* proofs in a pass dispatched while no pass is in flight (the
                           start of a job): default 4096, 0 = batch.  A smaller first
                           pass reaches the device after half the planning step: a
                           20-step bench job 707k -> 725k transfers/s (mean of 4 on one
                           box, profiles/r05/first_pass_ab.txt)                        */
  uint32_t tail_split;  /* the last pass of the queue (pending <= batch) is cut in two
                           halves of at least this many proofs, whose kernel chains then
                           overlap: 0 (default) = off (measured no gain on the 20-step
                           job, profiles/r05/tail_split_ab.txt)                         */
  uint32_t msm_graph;   /* 1: ftz_msm_run replays its launch chain (keys, sort, bucket,
                           segment, tree and Horner kernels) as one HIP graph captured on
                           the handle's first run; 0 (default): direct launches (the
                           graph measured the same: 2^16 0.92-0.93 ms either way,
                           profiles/r06/msm_graph.txt)                                   */
  uint32_t request_threads; /* threads decoding token requests (ftz_verify_token_requests*;
                           0 = threads): they share the host's cores with the planning
                           threads that feed the device                                  */
  uint32_t lookahead;   /* full passes (closed at the item or pair budget: a big call)
                           that may be planned, uploaded and enqueued behind a running
                           pass on its stream triple, so that the next pass's first kernel
                           starts the moment the running one ends and the host's plan and
                           enqueue time leave the device's critical path.  Costs one more
                           buffer set per triple and unit.  A partial
                           pass (small callers) still needs an idle triple.  Default 0
                           = off: at 1 the headline job was 3.3 % slower (0 of 5
                           pairs) -- the device is busy 99.9 % of that job already, and
                           a fourth concurrent pass only stretches the other three
                           (profiles/r09/ab_lookahead.txt, trace_gaps.txt)          */
} ftz_options;
#define FTZ_HOLD_NEVER 0xFFFFFFFFu
void ftz_options_default(ftz_options* opt);

/* pp: json(driver.SerializedPublicParameters{Identifier:"zkatdlog", Raw}) as
 * produced by crypto.PublicParams.Serialize (setup.go:119-128) and read by
 * PublicParams.Deserialize (setup.go:134-151) + Validate (setup.go:238-273).
 * device: HIP device ordinal (the local rank in a multi-GPU job). */
int ftz_ctx_create(const uint8_t* pp, size_t pp_len, int device, ftz_ctx** out);
int ftz_ctx_create_ex(const uint8_t* pp, size_t pp_len, int device, const ftz_options* opt, ftz_ctx** out);
/* Call only when no other call on the context is running. */
void ftz_ctx_destroy(ftz_ctx* ctx);
/* last error message of the calling thread (empty string if none) */
const char* ftz_last_error(void);
/* number of host threads used to plan a batch; only before the first
 * ftz_verify_* call on the context (FTZ_E_INVALID afterwards) */
int ftz_ctx_set_threads(ftz_ctx* ctx, int threads);
/* profiling: 1 = run every kernel of a batch on one stream (per-kernel times
 * without overlap), 0 = the normal three-stream schedule */
int ftz_ctx_set_serial(ftz_ctx* ctx, int serial);
/* testing the job engine's failure isolation: planning a device pass that
 * holds an item whose proof pointer equals `proof` fails (FTZ_E_INVALID,
 * "poisoned item"), as a planner limit would; NULL clears it.  The engine must
 * then deliver that error to the one request holding the item and the right
 * codes to every other caller whose items shared the pass. */
int ftz_ctx_debug_poison(ftz_ctx* ctx, const uint8_t* proof);
/* parity debugging: with FTZ_DEBUG_CHALLENGES set, batches loaded afterwards
 * (ftz_batch_load_*) keep every recomputed Fiat-Shamir challenge -- the
 * HashToZr of each well-formedness, membership and range transcript
 * (transfer/wellformedness.go, sigproof/membership.go:260-277,
 * range/proof.go:371-389) -- whether or not it matches the proof's claim.  Set
 * it before any call plans on the context; 0 clears it. */
#define FTZ_DEBUG_CHALLENGES 1
int ftz_ctx_set_debug(ftz_ctx* ctx, int flags);
/* profiling: kernel layout of a pipeline stage (results are identical; only
 * speed differs).  stage FTZ_STAGE_G2LINES (the verifier's t' = c PK0 + v PK1
 * + h PK2 and its 88 pair-2 Miller lines; default one lane) or
 * FTZ_STAGE_PROVER_G2LINES (the prover's t = rv PK1 + rh PK2 and its lines at
 * R'; default sextet); layout FTZ_LAYOUT_ONE_LANE (one lane per job) or
 * FTZ_LAYOUT_SEXTET (six lanes per job, ten jobs per wave). */
#define FTZ_STAGE_G2LINES 0
#define FTZ_STAGE_PROVER_G2LINES 1
#define FTZ_LAYOUT_ONE_LANE 1
#define FTZ_LAYOUT_SEXTET 6
int ftz_ctx_set_layout(ftz_ctx* ctx, int stage, int layout);
/* crypto.PublicParams.Validate (setup.go:238-273) on serialized public
 * parameters, as the FSC node's loader runs it (nogh/loaders.go:133):
 * FTZ_SUCCESS, or FTZ_E_PP with the reference's error text in
 * ftz_last_error().  Point encodings are checked by ftz_ctx_create. */
int ftz_pp_validate(const uint8_t* pp, size_t pp_len);
/* crypto.Setup (setup.go:214-236: pssign KeyGen(1), GeneratePedersenParameters
 * :153-166, GenerateRangeProofParameters :168-184 with the R = generator quirk of
 * pssign/sign.go:97-98, QuantityPrecision 64) followed by Serialize
 * (setup.go:119-128): out receives json(driver.SerializedPublicParameters) for
 * SignedValues of 0..base-1 and the given Exponent / IdemixIssuerPK (NULL: JSON
 * null) / IdemixCurveID.  The reference draws its scalars from crypto/rand;
 * here rand(tag) = SHA-256(seed||tag||0) || SHA-256(seed||tag||1) mod r, so a
 * seed reproduces a parameter set.  Host-side (once per network): no context
 * or GPU needed.  *out_len = the size; FTZ_E_INVALID if cap is too small. */
int ftz_pp_setup(uint64_t base, uint32_t exponent, const uint8_t* idemix_pk, size_t idemix_pk_len, int idemix_curve,
                 const uint8_t* seed, size_t seed_len, uint8_t* out, size_t cap, size_t* out_len);
/* the context's resolved options (threads, batch, slots, window, fexp) */
int ftz_ctx_options(const ftz_ctx* ctx, ftz_options* out);
/* PP properties: base (len(SignedValues)) and exponent */
int ftz_ctx_info(const ftz_ctx* ctx, uint32_t* base, uint32_t* exponent);

/* Verify n proofs (any n: large calls are split into device batches and
 * pipelined, small concurrent calls share batches); codes[i] receives FTZ_OK
 * or an FTZ_ERR_* class. */
int ftz_verify_transfers(ftz_ctx* ctx, size_t n, const ftz_transfer* tx, int32_t* codes);
int ftz_verify_issues(ftz_ctx* ctx, size_t n, const ftz_issue* is, int32_t* codes);

/* Job-engine counters since context creation (or the last reset): device
 * batches, proofs, host planning time (parse + layout into the pinned staging
 * blob), enqueue time (H2D copy + kernel launches), device time per batch
 * (HIP events from the H2D copy to the verdict download), and the caller-side
 * wait of the completion thread. */
typedef struct {
  uint64_t batches;
  uint64_t proofs;
  double plan_ms;    /* sum over batches */
  double submit_ms;  /* sum over batches */
  double device_ms;  /* sum over batches, upload -> verdicts downloaded */
  double wall_ms;    /* first submission -> last completion */
  uint32_t max_in_flight;  /* passes enqueued at once, running or queued behind one */
  uint32_t queued_ahead;   /* passes enqueued behind a running pass (ftz_options.lookahead) */
  uint32_t max_per_triple; /* most passes enqueued on one stream triple at once */
} ftz_engine_stats;
int ftz_ctx_engine_stats(ftz_ctx* ctx, ftz_engine_stats* out, int reset);
/* testing: the job engine's buffer sets.  caps receives, for each of at most
 * max_sets sets, the capacities in bytes of its pinned staging blob, device
 * blob, device scratch and pinned result buffer (4 values per set); *n_sets
 * the number of sets the engine owns (0 before the first ftz_verify_* call);
 * *partial_ahead how many partial passes were ever enqueued behind a running
 * one (the engine's rule keeps it 0 while slots <= 4).  Any pointer may be NULL. */
int ftz_ctx_debug_engine_sets(ftz_ctx* ctx, uint64_t* caps, size_t max_sets, size_t* n_sets, uint64_t* partial_ahead);

/* Host-side time of ftz_prove_transfers / ftz_prove_issues since context
 * creation (or the last reset), summed over device passes: waiting for a pass
 * to finish, copying its proofs into the caller's buffer, planning + flattening
 * the next pass into pinned staging, and enqueueing it (H2D copy + launches). */
typedef struct {
  uint64_t passes;
  uint64_t proofs;
  double wait_ms;
  double copy_ms;
  double plan_ms;
  double submit_ms;
  double wall_ms;    /* sum over calls, entry -> return */
} ftz_prover_host_stats;
int ftz_ctx_prover_stats(ftz_ctx* ctx, ftz_prover_host_stats* out, int reset);

/* Staged form: plan + upload once, then run the GPU pipeline on resident
 * inputs any number of times (used by bench.py to time the device path).
 * One staged batch is one device pass: n must keep every job pool of the
 * batch below 2^31 entries / bytes (FTZ_E_INVALID otherwise; a 2-in/2-out
 * PP-A transfer uses ~4 KB of arena, so up to ~500k transfers). */
int ftz_batch_load_transfers(ftz_ctx* ctx, size_t n, const ftz_transfer* tx, ftz_batch** out);
int ftz_batch_load_issues(ftz_ctx* ctx, size_t n, const ftz_issue* is, ftz_batch** out);
int ftz_batch_run(ftz_batch* b); /* = ftz_batch_submit + ftz_batch_wait */
/* Asynchronous form: enqueue the pipeline on the batch's own HIP streams and
 * return; several batches may be in flight at once (a validator pipelining
 * blocks).  ftz_batch_wait blocks until the batch's last submission is done
 * and records its ftz_stats; codes/bitmap wait implicitly.  A batch must not
 * be resubmitted before its previous submission was waited for. */
int ftz_batch_submit(ftz_batch* b);
int ftz_batch_wait(ftz_batch* b);
int ftz_batch_codes(ftz_batch* b, int32_t* codes);
/* verdict bitmap: bit i set <=> proof i accepted; (n+7)/8 bytes */
int ftz_batch_bitmap(ftz_batch* b, uint8_t* bits);
int ftz_batch_stats(const ftz_batch* b, ftz_stats* out);
size_t ftz_batch_size(const ftz_batch* b);
void ftz_batch_destroy(ftz_batch* b);
/* the recomputed challenges of proof i of a batch loaded with
 * FTZ_DEBUG_CHALLENGES, after ftz_batch_run: one per transcript the planner
 * scheduled, in check order -- well-formedness (FTZ_ERR_WF), then every
 * membership proof in (output, digit) order (FTZ_ERR_MEMBERSHIP), then the
 * range proof (FTZ_ERR_RANGE) -- as kinds[k] and 32-byte big-endian values at
 * values + 32 k.  *count = the number available (entries beyond cap are not
 * written).  A proof rejected before its transcripts are planned has none. */
int ftz_batch_challenges(ftz_batch* b, size_t i, int32_t* kinds, uint8_t* values, size_t cap, size_t* count);

/* ---- token commitments and auditor opening checks.
 * A token opening is token.TokenDataWitness{Type, Value, BlindingFactor}
 * (crypto/token/token.go): value and bf as 32-byte big-endian Zr.  The
 * commitment is H(type)*Ped0 + value*Ped1 + bf*Ped2 with H = HashToZr
 * (computeTokens, token/token.go:64-76; common/schnorr.go:59-76).  Note
 * GetTokensWithWitness (token.go:78-98) takes uint64 values through
 * NewZrFromInt(int64(v)): a caller passes that Zr (v mod r for v < 2^63). */
typedef struct {
  const char* type;
  size_t type_len;
  const uint8_t* value; /* 32 bytes */
  const uint8_t* bf;    /* 32 bytes */
} ftz_token_opening;
/* out: n x 64-byte RawBytes commitments */
int ftz_commit_tokens(ftz_ctx* ctx, size_t n, const ftz_token_opening* t, uint8_t* out);
/* Auditor InspectOutput / InspectInputs commitment check (audit/auditor.go:208-234):
 * codes[i] = FTZ_OK if commitments[i] (64-byte RawBytes, gnark decoding rules)
 * equals the recomputed commitment of t[i], FTZ_ERR_OPENING if it does not,
 * FTZ_ERR_PARSE if the bytes are not a valid G1 encoding.  (The owner
 * identity check InspectTokenOwnerFunc is idemix, outside this library.) */
int ftz_audit_openings(ftz_ctx* ctx, size_t n, const uint8_t* commitments, const ftz_token_opening* t,
                       int32_t* codes);

/* ---- Pointcheval-Sanders signature verification (crypto/pssign/sign.go:125-160
 * SignVerifier.Verify, for one message) against the context's SignPK / Q:
 *   H = PK0 + m PK1 + h PK2,  accept iff FExp(e(-S, Q) e(R, H)) is one in GT.
 * h is NOT recomputed (the reference's callers pass HashToZr(m.Bytes())).  m and
 * h are 32 big-endian bytes taken like every other Zr input (big.Int SetBytes,
 * then reduced mod r for scalar use): m + r verifies as m does.  r and s are
 * 64-byte gnark G1 encodings under the decoding rules of every other element
 * (flags, compressed forms, (0,0) = infinity, on-curve check).  A pair holding
 * a point at infinity is skipped by the Miller loop, as everywhere in this
 * library [EXT]: R = S = O is accepted, R = O alone (S != O) is rejected.
 * codes[i] = FTZ_OK (the reference returns nil), FTZ_ERR_PARSE (r or s does
 * not decode) or FTZ_ERR_PS_SIGNATURE.  Thread-safe; any n (tiled into passes
 * of at most 4 x ftz_options.batch items); n = 0 succeeds. */
#define FTZ_ERR_PS_SIGNATURE 14 /* invalid Pointcheval-Sanders signature */
typedef struct {
  uint8_t m[32], h[32], r[64], s[64];
} ftz_ps_sig;
int ftz_verify_ps_signatures(ftz_ctx* ctx, size_t n, const ftz_ps_sig* sigs, int32_t* codes);
/* Audit of RangeProofParams.SignedValues: entry i must be a signature on m = i
 * with h = HashToZr(32-byte big-endian i), which is what
 * GenerateRangeProofParameters signs (setup.go:168-184).  Always writes *count
 * = len(SignedValues); with cap >= *count, codes[i] = FTZ_OK or
 * FTZ_ERR_PS_SIGNATURE -- also for an entry whose R or S is the point at
 * infinity, which the item call above would skip (an audit has no reference
 * behaviour to mirror).  cap < *count: FTZ_E_INVALID after writing *count.
 * Neither ftz_pp_validate nor ftz_ctx_create runs this check. */
int ftz_pp_audit_signed_values(ftz_ctx* ctx, int32_t* codes, size_t cap, size_t* count);

/* ---- raw token requests (the wire format around the path).
 * A request is asn1.Marshal(driver.TokenRequest{Issues, Transfers, Signatures,
 * AuditorSignatures [][]byte}) (token/driver/request.go:24-38). */
typedef struct {
  const uint8_t* p;
  size_t len;
} ftz_bytes;
/* Go encoding/asn1 decoding as TokenRequest.FromBytes does it (request.go:35-38):
 * counts[0..3] = len(Issues), len(Transfers), len(Signatures), len(AuditorSignatures);
 * elems[0 .. sum(counts)) receive the byte slices in that order, pointing into
 * raw (when cap is large enough).  FTZ_SUCCESS, or FTZ_E_INVALID for bytes
 * the reference rejects (message in ftz_last_error) or a too small cap. */
int ftz_token_request_decode(const uint8_t* raw, size_t len, size_t counts[4], ftz_bytes* elems, size_t cap);
/* Ledger lookup (driver.GetStateFnc, validator.go:45; the Go shim passes a cgo
 * export over getState): 0 and *val / *val_len (valid until the next call on
 * the same thread), or non-zero when the state cannot be read.  Called on the
 * thread that called ftz_verify_token_requests only, never concurrently; the
 * library copies each value before the next call. */
typedef int (*ftz_get_state_fn)(void* user, const char* key, size_t key_len, const uint8_t** val, size_t* val_len);
/* Batched ledger lookup (one cgo crossing per pipeline chunk instead of one per
 * input): vals[i] = the value of keys[i], {NULL, 0} when it does not exist.
 * Returns 0, or non-zero when the states cannot be read (every transfer with
 * an input in this call then fails with FTZ_ERR_INPUT, as a GetState error
 * does).  Called on the thread that called ftz_verify_token_requests_batched
 * only, never concurrently; the values must stay valid until the next
 * get_states call or the return of ftz_verify_token_requests_batched (the
 * library copies them before either).  The Go side may look the keys up
 * concurrently itself. */
typedef int (*ftz_get_states_fn)(void* user, size_t n, const ftz_bytes* keys, ftz_bytes* vals);
#define FTZ_ERR_INPUT 8 /* an input to spend is missing on the ledger or is not a token.Token */
/* ZK validation of n raw token requests as Validator.VerifyTokenRequestFromRaw
 * performs it (crypto/validator/validator.go:45-108) minus the checks that stay
 * in Go (auditor / issuer / owner signatures, HTLC scripts, metadata counting):
 * ASN.1 and action JSON decoding (a failure rejects the whole request with
 * FTZ_ERR_PARSE, as unmarshalIssueActions / unmarshalTransferActions do), then
 * every issue action (issue.Verifier) and every transfer action (inputs loaded
 * through get_state and decoded as token.Token -- FTZ_ERR_INPUT --, then
 * transfer.Verifier) in order; all actions of all requests are verified in
 * shared device batches.  codes[i] = FTZ_OK or the first failing check of
 * request i; failed_action (may be NULL) = that action's index (issues first,
 * then transfers), -1 if none or request-level.
 * Pipelined: requests are decoded on the library's own host threads in chunks,
 * and while chunk k's actions are verified on the device, chunk k+1 is decoded
 * and its inputs looked up (on the calling thread).  Thread-safe: calls on one
 * context from several threads share the device batches. */
int ftz_verify_token_requests(ftz_ctx* ctx, size_t n, const ftz_bytes* reqs, ftz_get_state_fn get_state, void* user,
                              int32_t* codes, int32_t* failed_action);
/* The same with the batched ledger lookup (recommended for block-level
 * binding: one callback per pipeline chunk of up to 4096 requests). */
int ftz_verify_token_requests_batched(ftz_ctx* ctx, size_t n, const ftz_bytes* reqs, ftz_get_states_fn get_states,
                                      void* user, int32_t* codes, int32_t* failed_action);
/* profiling: the calling thread's time in each stage of the request pipeline,
 * summed over the context's ftz_verify_token_requests* calls, in ms: ms[0]
 * decode (ASN.1 + action JSON, parallel), [1] element checks (device), [2]
 * ledger callbacks, [3] token decoding (parallel), [4] job building, [5]
 * waiting for the verdicts of earlier chunks; reset != 0 zeroes them after. */
int ftz_ctx_request_stats(ftz_ctx* ctx, double ms[6], int reset);

/* ---- idemix owner signatures, on BN254 or FP256BN_AMCL.
 * Replaces, per input token of a transfer, what TransferSignatureValidate
 * (crypto/validator/validator_transfer.go:42-82) runs after loading the token:
 * ctx.Deserializer.GetOwnerVerifier(tok.Owner) (nogh/deserializer.go:64-66 ->
 * interop/htlc/deserializer.go:31-43 -> identity/owner.go:62-68 ->
 * identity/msp/idemix/deserializer.go:83-95, common.go:40-117) and
 * verifier.Verify(message, sigma) (common/backend.go:32-41 ->
 * identity/msp/idemix/deserializer.go:153-163 -> IBM/idemix NymSignature.Ver):
 * owner = the token's Owner bytes (ASN.1 RawOwner), msg = the signed request
 * bytes, sig = the NymSignature proto.  ftz_idemix_create takes
 * PublicParams.IdemixIssuerPK (setup.go:36) -- the IssuerPublicKey proto -- and
 * PublicParams.IdemixCurveID, which selects the translator as
 * identity/msp/idemix/deserializer.go:40-51 does: FTZ_CURVE_BN254 (1, the
 * curve cmd/pp/dlog/gen.go:117 and every NWO topology deploy: gurvy
 * translator, gnark point decoding, 64-byte G1 in the transcript) or
 * FTZ_CURVE_FP256BN_AMCL (0, amcl translator).  The IPK's own proof is checked
 * once by the Go deserializer (NewDeserializer) and is not re-checked here; an
 * IPK whose HSk / HRand do not decode on the curve, or are the point at
 * infinity, is refused with FTZ_E_PP. */
#define FTZ_ERR_OWNER 9        /* the owner identity does not deserialize (RawOwner, idemix identity, nym) */
#define FTZ_ERR_SIGNATURE 10   /* the signature does not unmarshal, or "pseudonym signature invalid"       */
#define FTZ_ERR_UNSUPPORTED 11 /* owner type verified in Go (an HTLC script owner)                          */
#define FTZ_ERR_AUDIT 12       /* the token owner does not match its audit info (AuditInfo.Match failed)    */
#define FTZ_CURVE_FP256BN_AMCL 0
#define FTZ_CURVE_BN254 1
typedef struct ftz_idemix ftz_idemix;
typedef struct {
  const uint8_t* owner; /* token.Token.Owner: asn1(RawOwner{Type, Identity})                  */
  size_t owner_len;
  const uint8_t* msg;   /* the signed message (request bytes || anchor)                        */
  size_t msg_len;
  const uint8_t* sig;   /* proto(NymSignature)                                                 */
  size_t sig_len;
} ftz_owner_sig;
int ftz_idemix_create(ftz_ctx* ctx, const uint8_t* ipk, size_t ipk_len, int curve_id, ftz_idemix** out);
/* codes[i] = FTZ_OK, FTZ_ERR_OWNER, FTZ_ERR_SIGNATURE or FTZ_ERR_UNSUPPORTED; thread-safe */
int ftz_verify_owner_signatures(ftz_idemix* ix, size_t n, const ftz_owner_sig* s, int32_t* codes);
/* Strict nym import (opt-in, default off; FP256BN only -- on BN254 gnark's
 * SetBytes already refuses an off-curve nym, FTZ_ERR_OWNER).  amcl NewECPbigs turns an off-curve
 * NymX/NymY into the point at infinity [EXT, unpinned: amcl is not in the
 * reference], and NymSignature.Ver then accepts a signature made against the
 * identity without any secret; parity with that reading is the default.  With
 * on != 0 an off-curve nym is FTZ_ERR_OWNER before any curve arithmetic (a
 * deliberate deviation from the reference, for deployments that prefer to
 * reject until the amcl behaviour is confirmed).  Applies to later calls. */
int ftz_idemix_set_strict_nym(ftz_idemix* ix, int on);
void ftz_idemix_destroy(ftz_idemix* ix);

/* Auditor owner inspection (the owner half of
 * crypto/audit/auditor.go:208-274 InspectOutput / InspectInputs ->
 * InspectTokenOwner): the idemix matcher of the token's OwnerInfo
 * (identity/msp/idemix/audit.go:32-46 DeserializeAuditInfo, Go encoding/json)
 * checks the owner identity (audit.go:51-83 AuditInfo.Match ->
 * CSP.Verify(EidNymAuditOpts) -> IBM/idemix AuditNymEid [EXT]:
 * HAttrs[2]^HashToZr(Attributes[2]) * HRand^RNymEid == the identity proof's
 * EidNym).  codes: FTZ_OK, FTZ_ERR_OWNER (redeem token, empty OwnerInfo,
 * undecodable RawOwner or audit info), FTZ_ERR_AUDIT (Match failed),
 * FTZ_ERR_UNSUPPORTED (a script owner: inspected in Go), FTZ_ERR_PANIC. */
typedef struct {
  const uint8_t* owner;      /* token.Token.Owner: asn1(RawOwner{Type, Identity}) */
  size_t owner_len;
  const uint8_t* audit_info; /* the owner's OwnerInfo: json(AuditInfo)           */
  size_t audit_info_len;
} ftz_owner_audit;
int ftz_audit_owners(ftz_idemix* ix, size_t n, const ftz_owner_audit* items, int32_t* codes);

/* Signing on the same handle, BN254 only: the owner's signature of each input
 * token of a transfer.  Replaces SigningIdentity.Sign
 * (identity/msp/idemix/id.go:195-210 -> CSP.Sign(UserKey, msg,
 * IdemixNymSignerOpts{Nym, IssuerPK}) -> IBM/idemix NewNymSignature) and, with
 * ftz_idemix_make_nyms, the pseudonym derivation MakeNym
 * (Nym = sk HSk + RNym HRand).  The reference draws r_sk, r_rnym and the nonce
 * from crypto/rand; here they are the output of an HMAC-SHA-256 DRBG (the
 * generator of RFC 6979, not that RFC's scheme: 512 bits reduced mod r per
 * value, bias below 2^-250, no retry loop) keyed with the user secret,
 * SHA-256(msg) and RNym, computed on the device and never copied to the host.
 * With `entropy` = NULL a signature is a function of (sk, RNym, Nym, msg); with
 * 32 bytes of fresh randomness the DRBG is seeded with
 * SHA-256(SHA-256(msg) || entropy) in place of SHA-256(msg) (a hedged nonce: a
 * repeated seed still cannot repeat the randomness across two messages).  So
 * the bytes differ from the reference's while every signature passes
 * NymSignature.Ver.  Up to 8 user secrets per handle, kept in device memory
 * (zeroed when the handle is destroyed); the library wipes its own host copies
 * of sk and RNym, the caller's buffers are the caller's to wipe.  Table
 * addresses depend on the secret scalars: for a process that owns its device.
 * The library does NOT check that `nym` belongs to (sk, RNym): a mismatched
 * nym gives a well-formed signature that does not verify;
 * ftz_idemix_make_nyms is how a caller derives matching nyms.  On an
 * FP256BN_AMCL handle the three calls return FTZ_E_INVALID (the device has no
 * scalar field for that curve).  Not wired into ftz_verify_token_requests. */
#define FTZ_IDEMIX_MAX_SIGNERS 8
#define FTZ_NYMSIG_LEN 136 /* proto(NymSignature): four fields of tag, length 0x20 and 32 bytes, always */
typedef struct {
  const uint8_t* msg;     /* hashed on the device                                            */
  size_t msg_len;
  int32_t signer;         /* index from ftz_idemix_add_signer                                */
  const uint8_t* r_nym;   /* 32 bytes big-endian, < r: the pseudonym's RNym                   */
  const uint8_t* nym;     /* 64 bytes: NymX || NymY as in SerializedIdemixIdentity            */
  const uint8_t* entropy; /* NULL, or 32 bytes of fresh randomness                            */
} ftz_nym_sign_item;
/* sk: the user secret, 32 bytes big-endian, 1 <= sk < r (else FTZ_E_INVALID, as
 * is a ninth signer). */
int ftz_idemix_add_signer(ftz_idemix* ix, const uint8_t sk[32], int32_t* signer);
/* sigs: n slots of FTZ_NYMSIG_LEN bytes.  codes[i] = FTZ_OK, or FTZ_ERR_OWNER
 * when `nym` is not a canonical finite point of the curve (a coordinate >= p,
 * (0, 0), or off the curve; checked on the host, the slot is zeroed, the other
 * items are unaffected).  An out-of-range signer, an r_nym >= r, a NULL r_nym
 * or nym, a NULL message with a non-zero length or a message over 512 MiB is
 * FTZ_E_INVALID for the call; thread-safe (one call at a time on the handle,
 * verification included). */
int ftz_sign_owner_signatures(ftz_idemix* ix, size_t n, const ftz_nym_sign_item* it, uint8_t* sigs, int32_t* codes);
/* nyms[i] = sk HSk + r_nyms[i] HRand as NymX || NymY (64 bytes; r_nyms: n x 32
 * bytes big-endian, each < r, else FTZ_E_INVALID for the call). */
int ftz_idemix_make_nyms(ftz_idemix* ix, int32_t signer, size_t n, const uint8_t* r_nyms, uint8_t* nyms);

/* ---- x509 ECDSA P-256 signatures: the auditor's signature of a request
 * (crypto/validator/validator.go:134-145), each issue action's issuer
 * signature (validator.go:170-176) and fabtoken owners.  Replaces
 * x509.MSPIdentityDeserializer.DeserializeVerifier (nogh/deserializer.go:56-57
 * -> identity/msp/x509/ecdsa.go:130-147: proto msp.SerializedIdentity, one PEM
 * block "PUBLIC KEY" or "CERTIFICATE") and edsaVerifier.Verify
 * (ecdsa.go:70-101: asn1 signature, SHA-256, the low-S rule, ecdsa.Verify) on
 * P-256 keys.  Identities that repeat across a block (the auditor, the issuers
 * of the public parameters) are registered once with ftz_ecdsa_add_identity --
 * at most 64 per handle, 510 KiB of device table each -- and named by index;
 * an identity seen once is passed with key = -1 and decoded per call.  Only
 * what is certain is decided here: FTZ_ERR_UNSUPPORTED means "verify this one
 * in Go" (another curve, an RSA key, another PEM block type, a PEM block not
 * in the canonical form, a certificate that departs from the expected DER
 * walk).  A certificate's own signature, validity and chain are not checked,
 * as in the reference; Go's x509.ParseCertificate is stricter than the walk to
 * the key done here, so register only identities the Go deserializer has
 * accepted (for the auditor and issuers: when the public parameters load).
 * ftz_verify_signed_token_requests (below) runs these checks inside the request
 * path; ftz_verify_token_requests does not. */
#define FTZ_ERR_IDENTITY 13 /* the identity does not deserialize to an ECDSA public key */
typedef struct ftz_ecdsa ftz_ecdsa;
typedef struct {
  const uint8_t* identity; /* proto(msp.SerializedIdentity); read when key < 0           */
  size_t identity_len;
  int32_t key;             /* >= 0: a registered key; -1: decode `identity`               */
  const uint8_t* msg;      /* the signed message (hashed on the device)                   */
  size_t msg_len;
  const uint8_t* sig;      /* DER ECDSA signature                                         */
  size_t sig_len;
} ftz_ecdsa_sig;
int ftz_ecdsa_create(ftz_ctx* ctx, ftz_ecdsa** out);
/* Decode the identity and build its table: *key = its index (the same identity
 * bytes give the same index again).  FTZ_E_INVALID (reason in ftz_last_error)
 * for an undecodable or unsupported identity and beyond 64 keys. */
int ftz_ecdsa_add_identity(ftz_ecdsa* e, const uint8_t* id, size_t id_len, int32_t* key);
/* codes[i] = FTZ_OK, FTZ_ERR_IDENTITY, FTZ_ERR_UNSUPPORTED or FTZ_ERR_SIGNATURE;
 * an out-of-range key is FTZ_E_INVALID for the call; thread-safe */
int ftz_verify_ecdsa_signatures(ftz_ecdsa* e, size_t n, const ftz_ecdsa_sig* s, int32_t* codes);
/* Host only: the identity's P-256 public key as X || Y (32 bytes big-endian
 * each).  Returns the per-item code (FTZ_OK, FTZ_ERR_IDENTITY,
 * FTZ_ERR_UNSUPPORTED; the reason in ftz_last_error) or FTZ_E_INVALID. */
int ftz_x509_public_key(const uint8_t* id, size_t id_len, uint8_t xy[64]);

/* Signing on the same handle: the auditor's endorsement of a request
 * (crypto/audit/auditor.go:118-135 Endorse -> Signer.Sign) and the issuers'
 * signatures.  Replaces edsaSigner.Sign (identity/msp/x509/ecdsa.go:50-64):
 * SHA-256, ecdsa.Sign, ToLowS, DER.  The nonce is RFC 6979's (HMAC-SHA-256 DRBG
 * over the private key and the digest), computed on the device and never
 * copied to the host.  With `entropy` = NULL a signature is a function of key
 * and message; with 32 bytes of fresh randomness they enter as RFC 6979 3.6's
 * additional data (a hedged nonce: a repeated seed still cannot repeat a nonce
 * across two messages).  Go's ecdsa.Sign draws its nonce at random, so the
 * bytes differ from the reference's; every signature passes edsaVerifier.Verify
 * (minimal DER, 1 <= r < n, 1 <= s <= (n-1)/2).  Up to 8 private scalars per
 * handle, kept in device memory (zeroed when the handle is destroyed); the
 * library wipes its own host copy, the caller's buffer is the caller's to wipe.
 * Table addresses depend on the nonce: for a process that owns its device.
 * Not wired into ftz_verify_token_requests. */
#define FTZ_ECDSA_MAX_SIGNERS 8
#define FTZ_ECDSA_SIG_MAX 72 /* stride of the output; a low-S P-256 DER signature is <= 71 bytes */
typedef struct {
  const uint8_t* msg;     /* hashed on the device                                       */
  size_t msg_len;
  int32_t signer;         /* index from ftz_ecdsa_add_signer                            */
  const uint8_t* entropy; /* NULL, or 32 bytes of fresh randomness mixed into the nonce */
} ftz_ecdsa_sign_item;
/* d: the private scalar, 32 bytes big-endian, 1 <= d < n (else FTZ_E_INVALID, as
 * is a ninth signer).  public_xy (may be NULL) receives d G as X || Y, computed
 * on the host, to build or check the signer's identity. */
int ftz_ecdsa_add_signer(ftz_ecdsa* e, const uint8_t d[32], int32_t* signer, uint8_t public_xy[64]);
/* sigs: n slots of FTZ_ECDSA_SIG_MAX bytes, sig_lens[i] of them written (the
 * rest zero).  codes[i] = FTZ_OK; the one exception is FTZ_ERR_SIGNATURE
 * (sig_lens[i] = 0) when r = 0 or s = 0, which has probability about 2^-256
 * and which no known input reaches.  An out-of-range signer, a NULL message
 * with a non-zero length or a message over 512 MiB is FTZ_E_INVALID for the
 * call; thread-safe (one call at a time on the handle, verification included). */
int ftz_sign_ecdsa(ftz_ecdsa* e, size_t n, const ftz_ecdsa_sign_item* it, uint8_t* sigs, uint32_t* sig_lens,
                   int32_t* codes);
void ftz_ecdsa_destroy(ftz_ecdsa* e);

/* ---- token requests with their signatures: Validator.VerifyTokenRequestFromRaw
 * (crypto/validator/validator.go:45-108) with the auditor's, the issuers' and
 * the owners' signatures beside the proofs; HTLC scripts and metadata counting
 * stay in Go.  One verdict per request: the first check that fails in the
 * reference's order.
 *
 * Signed message of a request: asn1.Marshal(TokenRequest{Issues, Transfers}) ||
 * binding (validator.go:57-66) -- the first two fields of `raw` as they stand
 * (the decoder accepts minimal DER only) under a recomputed outer header,
 * followed by 30 00 30 00 for the two nil slices; trailing bytes and extra
 * fields of `raw` never enter it.  Signature list (common/backend.go:32-40):
 * AuditorSignatures ++ Signatures when len(auditor) != 0, else Signatures; each
 * check below consumes the next one, a check that finds the list exhausted
 * fails with FTZ_ERR_SIGNATURE, left-over signatures are ignored.
 *
 *   1  empty request, ASN.1 (:46-53)                              FTZ_ERR_PARSE, -1
 *   2  auditor != NULL: its identity decodes (:136-139), the next signature
 *      verifies (:141)            FTZ_ERR_IDENTITY / _UNSUPPORTED / _SIGNATURE, -1
 *   3  every issue action, then every transfer action, unmarshals (:83-90)
 *                                                                 FTZ_ERR_PARSE, -1
 *   4  issue k: the proof checks of ftz_verify_token_requests (:151)
 *   5  issue k: Issuer is byte-equal to one of `issuers`, if any (:155-168)
 *                                                                 FTZ_ERR_ISSUER
 *   6  issue k: the issuer's identity decodes, the next signature verifies
 *      (:170-176)                 FTZ_ERR_IDENTITY / _UNSUPPORTED / _SIGNATURE
 *   7  transfer t, input j (validator_transfer.go:50-76): the state loads and is
 *      a token.Token                                              FTZ_ERR_INPUT
 *   8  the same input: its Owner gives a verifier
 *                                   FTZ_ERR_OWNER; a script owner FTZ_ERR_UNSUPPORTED
 *   9  the same input: the next signature verifies                FTZ_ERR_SIGNATURE
 *  10  transfer t: the proof checks of ftz_verify_token_requests
 *
 * Rows 4-6 are finished for issue k before issue k + 1; rows 7-9 run per input,
 * all inputs of a transfer before its proof.  A non-NULL auditor of length 0 is
 * Go's empty non-nil slice: row 2 runs and fails with FTZ_ERR_IDENTITY.
 * FTZ_ERR_UNSUPPORTED takes its place in the order like a failure and means
 * "hand this request to Go".  failed_action as for ftz_verify_token_requests.
 *
 * The auditor and every issuers[i] are registered on `ec` with
 * ftz_ecdsa_add_identity on first use (more than 64 keys on the handle:
 * FTZ_E_INVALID for the call; an identity the handle cannot decode or does not
 * support fails only the requests that need it).  With n_issuers = 0 an issuer
 * is decoded per item.  All proof and signature checks of a pipeline chunk run
 * side by side, the signatures on the handles' own streams; the verdicts are
 * merged on the host.  Thread-safe like ftz_verify_token_requests_batched;
 * get_states is called under the same rules. */
#define FTZ_ERR_ISSUER 15 /* an issue action's Issuer is not among the public parameters' Issuers */
typedef struct {
  ftz_idemix* ix;            /* owner signatures; NULL: any transfer input is FTZ_ERR_UNSUPPORTED */
  ftz_ecdsa* ec;             /* auditor / issuer signatures; NULL likewise for those               */
  const uint8_t* auditor;    /* PublicParams.Auditor; NULL = nil (no auditor check).  Non-NULL with */
  size_t auditor_len;        /* length 0 = Go's empty non-nil slice (row 2 fails)                   */
  const ftz_bytes* issuers;  /* PublicParams.Issuers; n_issuers = 0: any issuer is admitted         */
  size_t n_issuers;
} ftz_request_signers;
typedef struct {
  ftz_bytes raw;
  ftz_bytes binding; /* the txID string */
} ftz_signed_request;
int ftz_verify_signed_token_requests(ftz_ctx* ctx, const ftz_request_signers* signers, size_t n,
                                     const ftz_signed_request* reqs, ftz_get_states_fn get_states, void* user,
                                     int32_t* codes, int32_t* failed_action);

/* ---- standalone BN254 G1 multi-scalar multiplication (BASELINE configs[2]):
 * out = sum_i k_i P_i as 64-byte gnark RawBytes.  Points: n x 64-byte
 * uncompressed RawBytes (must be canonical and on the curve); scalars: n x 32
 * bytes big-endian, reduced mod r.  The reference path has no MSM; this is the
 * operation mathlib exposes from gnark-crypto as G1Jac.MultiExp.  Pippenger
 * with signed windows over GLV half-scalars (k = k1 + k2 lambda, |k_i| < 2^128,
 * points P_i and phi(P_i)), c = floor(log2(2n) / 2) + 7 clamped to [8, 20].
 * Sizes: n in [1, 2^28], and windows x 2n < 2^30 sort entries (n up to
 * ~2^26; FTZ_E_INVALID beyond), or windows x 2n < 2^31 resident points with
 * msm_precompute. */
typedef struct ftz_msm ftz_msm;
int ftz_msm_g1(ftz_ctx* ctx, size_t n, const uint8_t* points, const uint8_t* scalars, uint8_t out[64]);
/* staged form: upload once, run on HBM-resident inputs (bench) */
int ftz_msm_load(ftz_ctx* ctx, size_t n, const uint8_t* points, const uint8_t* scalars, ftz_msm** out);
/* test/bench inputs with known discrete logs: P_i = (i + offset) G generated on the device */
int ftz_msm_load_gen(ftz_ctx* ctx, size_t n, uint32_t offset, const uint8_t* scalars, ftz_msm** out);
int ftz_msm_run(ftz_msm* m, uint8_t out[64]);
/* replace the scalars of a loaded MSM (n x 32 bytes big-endian); the points, and
 * with msm_precompute their window multiples, stay resident */
int ftz_msm_set_scalars(ftz_msm* m, const uint8_t* scalars);
/* set the scalars and run in one call, for scalars that start in host memory:
 * the 32n bytes are copied in chunks on a copy stream while the key kernel of
 * the chunks already on the device runs (big-endian -> reduced limbs -> GLV
 * halves -> window digits in one pass), then the rest of ftz_msm_run.  The
 * scalars stay loaded, as with ftz_msm_set_scalars.  Page-locked memory
 * (ftz_host_alloc) copies at the full link rate. */
int ftz_msm_run_scalars(ftz_msm* m, const uint8_t* scalars, uint8_t out[64]);
/* page-locked host memory for staging large inputs (scalars, proof bytes) */
int ftz_host_alloc(size_t bytes, void** out);
void ftz_host_free(void* p);
/* device time of the last ftz_msm_run in ms (HIP events) and the window size */
int ftz_msm_info(const ftz_msm* m, float* last_ms, uint32_t* window_bits);
void ftz_msm_destroy(ftz_msm* m);
/* Sum of n <= 4096 RawBytes G1 points (the identity = 64 zero bytes accepted):
 * the final add of a point-split multi-GPU MSM: each rank runs
 * ftz_msm_g1 on its contiguous slice of the points, the 64-byte partials are
 * all-gathered (RCCL), and every rank sums them here (zkatdlog/dist.py msm_shard). */
int ftz_g1_sum(ftz_ctx* ctx, size_t n, const uint8_t* points, uint8_t out[64]);

/* ---- batch prover (BASELINE configs[4]).
 * Replaces transfer.NewProver(inW, outW, in, out, pp).Prove()
 * (token/core/zkatdlog/crypto/transfer/transfer.go:42,89-121) and
 * issue.NewProver(...).Prove() (crypto/issue/issue.go:151,162-184): the proof
 * JSON bytes, byte-identical to the reference's encoding.  Witnesses follow
 * token.TokenDataWitness (crypto/token/token.go): Value and BlindingFactor as
 * 32-byte big-endian Zr.  Randomness: the reference draws from crypto/rand;
 * here every random scalar is SHA-256(seed||tag||0)||SHA-256(seed||tag||1) mod r
 * from a caller-supplied 32-byte seed per proof (the Go shim passes 32 bytes of
 * crypto/rand), so proofs are reproducible for testing.  A value outside
 * [0, base^exponent) fails the load with FTZ_E_INVALID ("can't compute range
 * proof: value of token outside authorized range", range/proof.go:300-302). */
typedef struct {
  const uint8_t* inputs;     /* n_in x 64-byte RawBytes (ledger input commitments) */
  uint32_t n_in;
  const uint8_t* outputs;    /* n_out x 64-byte RawBytes (output commitments)      */
  uint32_t n_out;
  const uint8_t* in_values;  /* n_in x 32-byte BE Zr                               */
  const uint8_t* in_bfs;     /* n_in x 32-byte BE Zr                               */
  const uint8_t* out_values; /* n_out x 32-byte BE Zr                              */
  const uint8_t* out_bfs;    /* n_out x 32-byte BE Zr                              */
  const char* type;          /* token type (TokenDataWitness.Type)                 */
  size_t type_len;
  const uint8_t* seed;       /* 32 bytes                                           */
} ftz_transfer_witness;
typedef struct {
  const uint8_t* outputs;    /* n_out x 64-byte RawBytes (issued commitments)      */
  uint32_t n_out;
  const uint8_t* values;     /* n_out x 32-byte BE Zr                              */
  const uint8_t* bfs;        /* n_out x 32-byte BE Zr                              */
  const char* type;
  size_t type_len;
  uint8_t anonymous;
  const uint8_t* seed;       /* 32 bytes                                           */
} ftz_issue_witness;
typedef struct ftz_prover ftz_prover;
/* one call: proofs concatenated into buf (cap bytes; ftz_prover_bytes tells the
 * size), offsets[n+1] delimit proof i; codes[i] = FTZ_ERR_PARSE if a commitment
 * of proof i does not decode, else FTZ_OK */
int ftz_prove_transfers(ftz_ctx* ctx, size_t n, const ftz_transfer_witness* w, uint8_t* buf, size_t cap,
                        size_t* offsets, int32_t* codes);
int ftz_prove_issues(ftz_ctx* ctx, size_t n, const ftz_issue_witness* w, uint8_t* buf, size_t cap,
                     size_t* offsets, int32_t* codes);
/* staged form: plan + upload once, run on HBM-resident witnesses (bench) */
int ftz_prover_load_transfers(ftz_ctx* ctx, size_t n, const ftz_transfer_witness* w, ftz_prover** out);
int ftz_prover_load_issues(ftz_ctx* ctx, size_t n, const ftz_issue_witness* w, ftz_prover** out);
int ftz_prover_run(ftz_prover* p); /* = ftz_prover_submit + ftz_prover_wait */
/* asynchronous form on the prover's own streams (as ftz_batch_submit / ftz_batch_wait) */
int ftz_prover_submit(ftz_prover* p);
int ftz_prover_wait(ftz_prover* p);
size_t ftz_prover_bytes(const ftz_prover* p);
int ftz_prover_proofs(ftz_prover* p, uint8_t* buf, size_t cap, size_t* offsets, int32_t* codes);
int ftz_prover_stats(const ftz_prover* p, ftz_stats* out);
void ftz_prover_destroy(ftz_prover* p);

/* ---- actions from cleartext values in one call.
 * Replaces Sender.GenerateZKTransfer (crypto/transfer/sender.go:52-88) and the
 * non-anonymous Issuer.GenerateZKIssue (crypto/issue/nonanonym/nonanonymissuer.go:
 * 37-80): values and owners in, json.Marshal of the action and one
 * json.Marshal(token.Metadata) per output out.  Everything the reference draws
 * from crypto/rand comes from the order's 32-byte seed as in ftz_prove_*: output
 * k's blinding factor is rand("tx/token/bf/<k>") for a transfer and
 * rand("issue/token/bf/<k>") for an issue, its commitment is H(type) Ped0 +
 * value Ped1 + bf Ped2, and the proof is the one ftz_prove_* returns for that
 * witness and seed.  The commitments, the proof, the action and the metadata
 * documents are all written on the device.
 *   transfer action: {"Inputs":[ids],"InputCommitments":[canonical RawBytes of the
 *     decoded inputs],"OutputTokens":[{"Owner","Data"}],"Proof","Metadata":{}}
 *   issue action: {"Issuer","outputs":[{"Owner","Data"}],"Proof","Anonymous":false,
 *     "Metadata":null}
 *   metadata: {"Type","Value","BlindingFactor","Owner","Issuer"}, Issuer null for
 *     a transfer
 * Refused with FTZ_E_INVALID and a message naming the order: no inputs, no
 * outputs, a null seed, a context whose exponent is <= 0, a type or id that is
 * not valid UTF-8 (Go would write U+FFFD and the action would not round-trip), an
 * output value >= 2^63 ([EXT]: NewZrFromInt(int64(v)) is negative there), and --
 * except for the 1-in/1-out transfer, which has no range proof -- a value >=
 * base^exponent, as ftz_prove_* refuses it.  The sum of inputs and outputs is not
 * checked, as in the reference; the verifier rejects an unbalanced action. */
typedef struct {
  const ftz_bytes* input_ids;  /* n_in ledger keys (TransferAction.Inputs), UTF-8           */
  const uint8_t* inputs;       /* n_in x 64-byte G1 (the ledger tokens' Data), gnark rules  */
  uint32_t n_in;
  const uint8_t* in_values;    /* n_in x 32-byte BE Zr (the inputs' token.Metadata)         */
  const uint8_t* in_bfs;       /* n_in x 32-byte BE Zr                                      */
  const uint64_t* out_values;  /* n_out (GenerateZKTransfer takes []uint64)                 */
  const ftz_bytes* out_owners; /* n_out; p == NULL: Go nil (JSON null), p != NULL && len == 0: "" */
  uint32_t n_out;
  const char* type;
  size_t type_len;
  const uint8_t* seed;         /* 32 bytes, as ftz_transfer_witness.seed                    */
} ftz_transfer_order;
typedef struct {
  ftz_bytes issuer;            /* Signer.Serialize(); NULL / empty as for owners            */
  const uint64_t* values;      /* n_out                                                     */
  const ftz_bytes* owners;     /* n_out                                                     */
  uint32_t n_out;
  const char* type;
  size_t type_len;
  const uint8_t* seed;         /* 32 bytes                                                  */
} ftz_issue_order;
/* Exact byte counts of the two buffers below, from the orders alone (every
 * document has a fixed length given the lengths of its strings). */
int ftz_generate_transfers_size(ftz_ctx* ctx, size_t n, const ftz_transfer_order* o, size_t* action_bytes,
                                size_t* meta_bytes);
int ftz_generate_issues_size(ftz_ctx* ctx, size_t n, const ftz_issue_order* o, size_t* action_bytes,
                             size_t* meta_bytes);
/* One call: action i at actions[action_off[i] .. action_off[i+1]), the metadata of
 * output t (counted over all orders, T in total) at meta[meta_off[t] ..
 * meta_off[t+1]), its commitment (canonical RawBytes) at commitments + 64 t
 * (commitments may be NULL).  codes[i] = FTZ_ERR_PARSE when an input commitment of
 * order i does not decode: its action and metadata entries are then empty and
 * its commitment slots zero; other orders are unaffected.  A capacity that is too
 * small: FTZ_E_INVALID with the needed sizes in ftz_last_error (ask
 * ftz_generate_*_size first).  Runs through the slots, streams and host statistics
 * of ftz_prove_*; thread-safety is the same. */
int ftz_generate_transfers(ftz_ctx* ctx, size_t n, const ftz_transfer_order* o, uint8_t* actions, size_t action_cap,
                           size_t* action_off, uint8_t* meta, size_t meta_cap, size_t* meta_off,
                           uint8_t* commitments, int32_t* codes);
int ftz_generate_issues(ftz_ctx* ctx, size_t n, const ftz_issue_order* o, uint8_t* actions, size_t action_cap,
                        size_t* action_off, uint8_t* meta, size_t meta_cap, size_t* meta_off, uint8_t* commitments,
                        int32_t* codes);
/* The inverse of ftz_token_request_decode: minimal DER, exactly
 * asn1.Marshal(driver.TokenRequest{Issues, Transfers, Signatures,
 * AuditorSignatures}).  With the last two empty, followed by the txID, it is the
 * message ftz_verify_signed_token_requests rebuilds.  *len receives the length;
 * cap < *len (or out == NULL): FTZ_E_INVALID after writing *len. */
int ftz_token_request_encode(const ftz_bytes* issues, size_t n_issues, const ftz_bytes* transfers, size_t n_transfers,
                             const ftz_bytes* signatures, size_t n_signatures, const ftz_bytes* auditor_signatures,
                             size_t n_auditor_signatures, uint8_t* out, size_t cap, size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* FTSAMD_H */
