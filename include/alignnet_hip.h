/*
 * alignnet_hip.h -- C ABI of libalignnet_hip.so, the MI355X (gfx950) engine for the
 * AlignNet-3D `tp8` network.
 *
 * The reference (grossjohannes/AlignNet-3D) has no FFI: the seam its hot path sits
 * behind is the Python module API consumed by train.py plus tf.Session.run.  Each
 * entry point below names the reference call site it replaces (paths relative to the
 * reference repository root).  Plain C types only; row-major float32 everywhere.
 *
 * Ownership: the caller owns every buffer it passes in; the library owns device
 * memory, parameters and optimiser state behind the opaque handle.
 * Errors: every call returns 0 on success, non-zero on failure; the message is
 * available from alignnet_last_error().  (The reference asserts / raises and aborts:
 * train.py:55,143,216,251 -- the Python wrapper raises on a non-zero status.)
 * Threading: one handle per GPU/process, calls on a handle are serialised by the
 * caller (the reference issues one blocking sess.run at a time).
 */
#ifndef ALIGNNET_HIP_H
#define ALIGNNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIGNNET_MAX_WIDTHS 8
#define ALIGNNET_ABI_VERSION 1

typedef struct alignnet_handle alignnet_handle;

/* A conv / fc width list as written in the JSON configs (model.options). */
typedef struct {
  int32_t n;
  int32_t w[ALIGNNET_MAX_WIDTHS];
} alignnet_widths;

/* Everything models/tp8.py reads from `cfg` at graph-build time (tp8.py:10,14,98,154,
 * 307-308,318) plus what train.py:133-174,211-217 reads for the schedules/optimiser. */
typedef struct {
  int32_t abi_version;   /* must be ALIGNNET_ABI_VERSION */
  int32_t device;        /* HIP device ordinal (train.py:189 cfg.gpu_index) */
  int32_t num_points;    /* cfg.model.num_points */
  int32_t num_channels;  /* cfg.data.num_channels (3) */
  int32_t num_bins;      /* cfg.model.angles.num_bins */
  int32_t backbone;      /* 0 = "pointnet", 1 = "dgcnn" (cfg.model.backbone) */
  alignnet_widths s1_conv, s1_fc;   /* options.s1transformer = [conv, [fc, keep]] */
  alignnet_widths s2_conv, s2_fc;   /* options.s2transformer */
  alignnet_widths emb_conv;         /* options.embedding */
  alignnet_widths rem_fc;           /* options.remaining_transform_prediction[0] */
  float s1_keep, s2_keep, rem_keep; /* dropout keep_prob; <= 0 means "None" (tp8.py:80) */
  float angle_factor;               /* options.angle_factor */
  float early_stage_factor;         /* options.early_stage_factor */
  int32_t accept_inverted_angle;    /* cfg.model.angles.accept_inverted_angle */
  /* training (train.py:133-174,211-217) */
  int32_t batch_size;               /* cfg.training.batch_size (global, drives schedules) */
  int32_t ntrain;                   /* cfg.data.ntrain */
  float learning_rate;              /* cfg.training.learning_rate */
  int32_t lr_step;                  /* lr_extension.step */
  float lr_rate;                    /* lr_extension.rate */
  int32_t lr_per_epoch;             /* lr_extension.per == "epoch" */
  float bn_init, bn_rate, bn_clip;  /* bn_extension.{init,rate,clip} */
  int32_t bn_step;                  /* bn_extension.step */
  int32_t bn_per_epoch;             /* bn_extension.per == "epoch" */
  int32_t optimizer;                /* 0 = adam, 1 = momentum (train.py:211-216) */
  float momentum;                   /* cfg.training.optimizer.momentum */
  uint64_t seed;                    /* dropout / init RNG stream */
} alignnet_config;

/* The nine prediction tensors tf.Session.run returns in eval (train.py:448) minus the
 * summary: all float32, caller-allocated, any of them may be NULL to skip it.
 * B rows each; widths: centres/translations 3, logits 2*num_bins. */
typedef struct {
  float* pred_translations;            /* [B,3]   tp8.py:155 */
  float* pred_remaining_angle_logits;  /* [B,2nb] tp8.py:156 */
  float* pred_s1_pc1centers;           /* [B,3]   tp8.py:146 */
  float* pred_s1_pc2centers;           /* [B,3]   tp8.py:147 */
  float* pred_s2_pc1centers;           /* [B,3]   tp8.py:148 */
  float* pred_s2_pc2centers;           /* [B,3]   tp8.py:149 */
  float* pred_pc1angle_logits;         /* [B,2nb] tp8.py:150 */
  float* pred_pc2angle_logits;         /* [B,2nb] tp8.py:151 */
} alignnet_outputs;

/* The six label tensors of placeholder_inputs (tp8.py:16-22). */
typedef struct {
  const float* translations;  /* [B,3] */
  const float* rel_angles;    /* [B,1] */
  const float* pc1_centers;   /* [B,3] */
  const float* pc2_centers;   /* [B,3] */
  const float* pc1_angles;    /* [B,1] */
  const float* pc2_angles;    /* [B,1] */
} alignnet_labels;

/* The scalars a train-mode sess.run returns (train.py:368) + the 16 summaries of
 * tp8.py:336-353 in declaration order + the two schedule scalars (train.py:197,210). */
typedef struct {
  int64_t step;          /* value of `batch` after the update */
  float loss;            /* per_transform_loss, tp8.py:334 */
  float learning_rate;   /* train.py:155 */
  float bn_decay;        /* train.py:173 */
  float summaries[16];   /* tp8.py:336-353 */
} alignnet_step_result;

typedef struct {
  int64_t step;
  float learning_rate;
  float bn_decay;
} alignnet_state;

/* ---- lifetime: replaces graph construction, train.py:190-227 ------------------ */
int alignnet_create(const alignnet_config* cfg, alignnet_handle** out);
void alignnet_destroy(alignnet_handle* h);
/* Message of the most recent failure on this handle (h may be NULL for create()). */
const char* alignnet_last_error(const alignnet_handle* h);
int alignnet_abi_version(void);

/* ---- parameters: replaces sess.run(init) train.py:241 and tf.train.Saver
 *      get/set of individual variables (train.py:220,252,268,281) ----------------- */
int alignnet_init_params(alignnet_handle* h, uint64_t seed);   /* utils/tf_util.py:10-49 */
int alignnet_num_params(const alignnet_handle* h);
/* name: variable name (DESIGN.md section "variables"); rows*cols floats; trainable flag. */
int alignnet_param_info(const alignnet_handle* h, int index, const char** name,
                        int32_t* rows, int32_t* cols, int32_t* trainable);
int alignnet_get_param(alignnet_handle* h, const char* name, float* dst, size_t count);
int alignnet_set_param(alignnet_handle* h, const char* name, const float* src, size_t count);

/* ---- inference: replaces the eval sess.run, train.py:447-449 (is_training=False) -- */
/* Host buffers; any B >= 1 (no padding to a static batch needed, cf. train.py:451-452). */
int alignnet_forward(alignnet_handle* h, const float* pcs1, const float* pcs2, int32_t B,
                     const alignnet_outputs* out);
/* Device buffers already resident in HBM; asynchronous on the handle's stream.
 * Follow with alignnet_synchronize() before reading the outputs. */
int alignnet_forward_device(alignnet_handle* h, const float* d_pcs1, const float* d_pcs2,
                            int32_t B, const alignnet_outputs* d_out);
/* Pipelined form of alignnet_forward for a stream of batches (the evaluation loop of train.py:432-462 issues one blocking
 * sess.run per batch): submit() stages the batch in pinned memory and queues copy-in (copy stream), forward (compute stream) and
 * copy-out (a third stream), then returns; wait() blocks until the OLDEST submitted batch is complete and its outputs are in the
 * `out` buffers that were passed to its submit() (they must stay valid until then; pcs1 / pcs2 may be reused as soon as submit()
 * returns).  At most two batches in flight: the copy-in of batch i + 1 runs under the forward of batch i.  Same results as
 * alignnet_forward, bit for bit.  (alignnet_eval_loss refers to the most recently SUBMITTED batch.) */
int alignnet_forward_submit(alignnet_handle* h, const float* pcs1, const float* pcs2, int32_t B,
                            const alignnet_outputs* out);
int alignnet_forward_wait(alignnet_handle* h);
/* Eval-mode loss on the last forward's predictions (train.py:448 `loss` fetch). */
int alignnet_eval_loss(alignnet_handle* h, const alignnet_labels* labels, int32_t B,
                       float* loss, float summaries[16]);
int alignnet_synchronize(alignnet_handle* h);

/* ---- training: replaces the train sess.run, train.py:368 (is_training=True):
 *      forward with batch statistics, loss, backward, (all-reduce), Adam, EMA, step++ */
/* dropout_u: optional host array of uniforms [0,1) used for the dropout masks, laid out
 * [s1 tower0 | s2 tower0 | s1 tower1 | s2 tower1 | pair head], each B x last-hidden-width;
 * NULL = draw on the device from cfg.seed and the step counter.
 * Shapes: PointNet backbones of any depth (2 .. 6 conv layers, models/tp8.py:49-59), widths multiples of 8.  Three-layer stages with
 * widths multiples of 32, C1, C2 <= 128, C3 <= 1024 (every shipped dataset config) run the fused recompute kernels; any other stage
 * (e.g. the five-layer backbones of configs/default.json) runs the layer-by-layer path (fp32, hidden widths <= 256, last <= 4096);
 * backbone "dgcnn" (models/tp8.py:30-46, k = 20, 20 <= num_points <= 4096): [C1, C2, C3] with C1 in {32, 64}, C2 in {64, 128} (every
 * shipped config) runs the fused edge kernels; any other list of 2 .. 6 widths (multiples of 8, edge convs <= 256) runs the same
 * layer-by-layer path over the B N k edge rows (fp32).
 * Anything else fails with a message (alignnet_last_error), it is never run on a fallback. */
int alignnet_train_step(alignnet_handle* h, const float* pcs1, const float* pcs2,
                        const alignnet_labels* labels, int32_t B, const float* dropout_u,
                        alignnet_step_result* result, const alignnet_outputs* out);
/* Same step with inputs and labels already resident in HBM (device pointers inside d_labels); dropout
 * masks are drawn on the device.  result may be NULL to avoid the host synchronisation. */
int alignnet_train_step_device(alignnet_handle* h, const float* d_pcs1, const float* d_pcs2,
                               const alignnet_labels* d_labels, int32_t B, alignnet_step_result* result);
/* Split form used for data-parallel training: forward+backward only (gradients stay on
 * the device), then the optimiser.  alignnet_grad_buffer exposes the flat gradient
 * (device pointer, float count) for an external all-reduce when the built-in RCCL
 * communicator is not used. */
int alignnet_train_forward_backward(alignnet_handle* h, const float* pcs1, const float* pcs2,
                                    const alignnet_labels* labels, int32_t B,
                                    const float* dropout_u, alignnet_step_result* result,
                                    const alignnet_outputs* out);
int alignnet_grad_buffer(alignnet_handle* h, float** d_grad, size_t* count);
int alignnet_apply_gradients(alignnet_handle* h, float grad_scale);   /* consumes the gradient: the buffer reads zero afterwards */
/* Debug/parity: copy the flat gradient of one variable to the host. */
int alignnet_get_grad(alignnet_handle* h, const char* name, float* dst, size_t count);
/* Debug/parity: the uniforms the device-side dropout stream (tf.nn.dropout's random_uniform, utils/tf_util.py:554-575) draws at
 * the current step counter when dropout_u is NULL, in the layout of dropout_u; count = B * (4 * w_hidden + w_pair_hidden).
 * A step run with these uniforms passed explicitly is bit-identical to the step that draws them itself. */
int alignnet_debug_dropout_uniforms(alignnet_handle* h, int32_t B, float* dst, size_t count);
/* Test hook: the k-nearest-neighbour graph (k = 20, self included; the SET tf.nn.top_k selects, ties at the k-th distance to the
 * lower index; utils/tf_util_dgcnn.py:638-676) the last eval-mode forward of a dgcnn engine built: int32 [2B][num_points][20],
 * tower 1's B clouds first.  count = 2 * B * num_points * 20.  Order within a row: nearest first when the query's candidate list
 * has <= 64 survivors (the usual case); queries with more survivors (clustered / duplicated points: every batch resampled with
 * replacement from a cloud of fewer than about N / 64 points) emit two runs, each in point-index order: first the candidates strictly
 * nearer than the k-th distance, then those AT the k-th distance, lowest indices first, until k are listed -- the max over the k
 * neighbours is order-invariant, so compare rows as sets (sorted) where that can occur (tests/knn_select_ref.py check_rows). */
int alignnet_debug_knn_graph(alignnet_handle* h, int32_t* dst, size_t count);
/* Test hook: what the last TRAINING forward on this handle DECIDED -- the discontinuous choices of the graph.  A parity test pins
 * the oracle to them (after checking that each one is a maximum of the oracle's own values to within rounding), so that the rest of
 * the comparison is continuous (tests/test_fullsize_gpu.py, oracle/alignnet_torch.py `pinned`).  All int32, towers outermost
 * (tower 1's B clouds, then tower 2's), B = the batch of that call:
 *   ALIGNNET_DECISION_YAW_CLASS   (stage ignored)  [2][B]              decoded yaw class, models/tp8.py:296
 *   ALIGNNET_DECISION_POOL_POINT  stage 0..2       [2][B][C_last]      arg-max point of the max over points, utils/tf_util.py:350-373 / models/tp8.py:58
 *   ALIGNNET_DECISION_EDGE_SLOT   stage 0..2, dgcnn [2][B][N][C_edge]  arg-max neighbour slot of the max over k, models/tp8.py:42
 *   ALIGNNET_DECISION_KNN_GRAPH   (stage ignored), dgcnn [2][B][N][20] the neighbour table the step used (slot = position in the row)
 *   ALIGNNET_DECISION_ANGLE_CLASS stage = loss term 0 (tower 1), 1 (tower 2): [2][B]; 2 (pair): [2][B][B] -- the class tf_angle2class
 *                                 (models/tp8.py:193-199) put each target angle of the loss into, for the target and for target + pi (:286);
 *                                 the pair term's target is the [B, B] matrix of :327, entry (i, j) = labels of row i against the decoded yaws of
 *                                 column j.  The residual label res = sh - centre(class) is a sawtooth in the angle: an entry within a rounding of
 *                                 a class boundary lands on the other tooth in another evaluation (label off by 2 in units of pi / num_bins).
 * count must equal the element count of the requested array. */
#define ALIGNNET_DECISION_YAW_CLASS 0
#define ALIGNNET_DECISION_POOL_POINT 1
#define ALIGNNET_DECISION_EDGE_SLOT 2
#define ALIGNNET_DECISION_KNN_GRAPH 3
#define ALIGNNET_DECISION_ANGLE_CLASS 4
int alignnet_debug_train_decisions(alignnet_handle* h, int32_t kind, int32_t stage, int32_t* dst, size_t count);
/* Test hook: the SIGN every relu of the last training step saw (utils/tf_util.py:167-168,345-346), one byte (0 / 1) per element.  What the
 * decisions above leave undecided are these signs: a pre-activation within one rounding of zero is "on" in one evaluation and "off" in another,
 * and on a row that wins many max-pool channels that re-routes per cents of a weight column's gradient.  A parity test pins the oracle to the
 * masks too (y = bn(z) * mask, after checking that every disagreeing pre-activation is rounding-sized) and the whole step becomes a smooth
 * function of its inputs (oracle/alignnet_torch.py `pinned["relu"]`, tests/test_fullsize_gpu.py).  Towers outermost, as above:
 *   ALIGNNET_RELU_CONV  stage 0..2, layer l of the stage's conv stack (models/tp8.py:30-59):
 *        hidden layers                       [2][B][N][C_l]        (dgcnn edge convs: [2][B][N][20][C_l])
 *        dgcnn, last edge conv (l = n - 2)   [2][B][N][C_l]        at the winning neighbour slot (max and relu commute)
 *        last conv (l = n - 1)               [2][B][C_l]           at the winning point
 *   ALIGNNET_RELU_HEAD  stage 0..2 = s1 head, s2 head, pair head (models/tp8.py:75-82), hidden layer j: [2][B][C_j] ([B][C_j] for the pair head)
 * Stored activations are read back; activations the passes recompute from xyz (conv1 of the fused stages) are recomputed by the same
 * device functions from the frame, weights and batch statistics of that step and its point clouds (after alignnet_train_step_device:
 * the caller's device buffers, which must still hold that batch).  Call it after alignnet_train_forward_backward, before the optimiser
 * changes the parameters (alignnet_apply_gradients) and before the next step.  count must equal the element count
 * of the requested array. */
#define ALIGNNET_RELU_CONV 0
#define ALIGNNET_RELU_HEAD 1
int alignnet_debug_train_relu_mask(alignnet_handle* h, int32_t kind, int32_t stage, int32_t layer, uint8_t* dst, size_t count);
/* Test hook, bf16 step only (train_matmul_bf16, fused stages): the bf16-ROUNDED activations the last training step fed to its MFMA convs, as bf16
 * bits, towers outermost: layer 0 = h1 [2][B][N][C1] (input of the hidden conv; dgcnn: the lifted edge features [2][B][N][20][C1], input of the second edge
 * conv), layer 1 = h2 [2][B][N][C2] (input of the lift; dgcnn: the pooled edge features, input of the point conv).  Every rounding of an
 * operand to bf16 is a small decision of its own (2^-8 of the value, a billion per step): an oracle that models the operand rounding (oracle/alignnet_torch.py
 * `bf16_lift`) and takes THESE rounded values -- after checking each is one of the two bf16 neighbours of its own value -- is a smooth function of its inputs,
 * as with the decisions and signs above.  Same calling window as alignnet_debug_train_relu_mask. */
int alignnet_debug_train_rounded(alignnet_handle* h, int32_t stage, int32_t layer, uint16_t* dst, size_t count);
/* Test hook: the loss kernels ALONE, on given head outputs (tests/test_loss_gpu.py).  Everything the loss depends on is an argument -- B pairs, nb angle
 * bins, accept_inverted, the two factors -- so one handle serves any parametrisation, whatever its own configuration; the call stages its own buffers and
 * touches no state of the handle's workspaces.  It runs, unchanged and on the handle's stream, the decode of the stage-2 heads (models/tp8.py:117,294-301),
 * the loss with its gradient (:304-354) and the read-back of the label classes.  Host arrays, float32, towers outermost (tower 1's B rows, then tower 2's):
 *   in   o2 [2B][3 + 2 nb]  stage-2 head outputs (centre offset, class logits, residual logits), s1c [2B][3] stage-1 centres,
 *        o3 [B][3 + 2 nb]   pair head outputs; labels: all six tensors of alignnet_labels
 *   out  out[17]            the loss and the 16 summaries (order of alignnet_step_result.summaries)
 *        s2c [2B][3], theta [2B], pcls [2B]   stage-2 centres, decoded yaw and its arg-max class (first maximum wins)
 *        cls1, cls2 [2][B], cls_pair [2][B][B]   the class of every target angle (target, target + pi), as ALIGNNET_DECISION_ANGLE_CLASS lays them out.
 *                           Always in [0, nb): where the float32 quotient of tf_angle2class rounds up to nb (labels just below the wrap, some nb only)
 *                           the class is 0 and the residual stays as computed, so that (class, residual) names the label's angle modulo 2 pi.
 *        want_grad != 0:    d_s1c, d_s2c [2B][3], d_o2 [2B][3 + 2 nb], d_o3 [B][3 + 2 nb]: the gradient as the loss kernels leave it, in front of the
 *                           glue backward (d_s2c holds the pred_translations path; d_o2[:, :3] is zero)
 * Any output pointer may be NULL.  B < 1, nb < 1 or a NULL input or label tensor: error, nothing is launched. */
int alignnet_debug_loss(alignnet_handle* h, int32_t B, int32_t nb, int32_t accept_inverted, float early_stage_factor, float angle_factor,
                        int32_t want_grad, const float* o2, const float* s1c, const float* o3, const alignnet_labels* labels, float* out,
                        float* s2c, float* theta, int32_t* pcls, int32_t* cls1, int32_t* cls2, int32_t* cls_pair, float* d_s1c, float* d_s2c,
                        float* d_o2, float* d_o3);

/* ---- multi-GPU (not in the reference, which is single-device: train.py:189).
 *      One process per GPU; RCCL communicator over xGMI for the gradient all-reduce. */
int alignnet_comm_unique_id(uint8_t id[128]);
/* Id of a new IN-PROCESS loopback group (first bytes "ALN3LOOP"): alignnet_comm_init with such an id joins `world` handles of ONE
 * process on ONE device, each driven by its own host thread, into a communicator whose collectives are stream-ordered device copies /
 * sums with a host rendezvous (csrc/comm_loopback.h) instead of RCCL.  Every multi-rank code path of the engine -- sync_bn's per-layer
 * sums, global_loss's gathers, the bucketed gradient all-reduce -- then runs with DIFFERENT shards on a 1-GPU box (tests/test_loopback_gpu.py:
 * W = 2 / 8 ranks against one engine at the concatenated batch, BASELINE.json configs[3]).  All ranks must issue the same collectives in
 * the same order (as with RCCL); a rank that fails breaks the group, the others return an error instead of waiting. */
int alignnet_comm_loopback_id(uint8_t id[128]);
int alignnet_comm_init(alignnet_handle* h, int32_t rank, int32_t world, const uint8_t id[128]);
/* Optional: a SECOND communicator of the same ranks (its own id, same rank / world as the first) that carries the gradient buckets
 * only.  NCCL-style communicators serialise the collectives issued on them across streams; with sync_bn a per-layer sum of the next
 * stage's backward would otherwise queue behind the previous stage's gradient bucket.  Results are identical with and without it
 * (tests/test_loopback_gpu.py); alignnet_get_option("grad_communicator") reads 1 when it exists.
 * HAZARD (why it is opt-in and off in bench.py): two RCCL communicators then have collectives in flight on two streams of one device at the
 * same time.  NCCL / RCCL document that as deadlock-prone when the device-side execution order of the two collectives differs between ranks
 * (each needs all ranks' kernels resident to progress).  It has run on the in-process loopback backend only, never on real links: validate it
 * on a multi-GPU node before relying on it. */
int alignnet_comm_init_grad(alignnet_handle* h, int32_t rank, int32_t world, const uint8_t id[128]);
int alignnet_comm_allreduce_grads(alignnet_handle* h);
/* Average the BatchNorm EMA shadows (the non-trainable variables) over the ranks, on the device: local-BN data parallelism updates them
 * from each rank's own shard (utils/tf_util.py:476-485); the drop-in train.py calls this once per epoch so that every rank's eval-mode
 * model and rank 0's checkpoint agree.  (Identical already under "sync_bn".) */
int alignnet_comm_average_shadows(alignnet_handle* h);

/* ---- schedule read-back: sess.run([learning_rate, bn_decay]) train.py:298,
 *      sess.run(batch) train.py:261,272 */
int alignnet_get_state(alignnet_handle* h, alignnet_state* st);
int alignnet_set_step(alignnet_handle* h, int64_t step);

/* ---- checkpoints: saver.save / saver.restore, train.py:252,268,281,317,321.
 *      Own container format; skip_step mirrors the pre-training restore
 *      that excludes `batch` (train.py:278-281). */
int alignnet_save(alignnet_handle* h, const char* path);
int alignnet_load(alignnet_handle* h, const char* path, int32_t skip_step);

/* ---- measurement hook for bench.py: HIP-event time (ms) of the dominant kernel
 *      (the fused shared-MLP backbone) accumulated since the last reset, and the
 *      number of launches, measured on the handle's own stream. */
int alignnet_profile_enable(alignnet_handle* h, int32_t on);

/* ---- HBM-resident dataset + device-side batch sampler ------------------------------
 * Replaces provider.load_batch (provider.py:85-136: per-example file opens, np.random.choice(n, N, replace=True)
 * resampling :97-98) and provider.jitter_point_cloud (provider.py:60-71, called at train.py:354-356) for runs that do
 * not need np.random's stream: the packed dataset is uploaded once and a batch is drawn on the device.
 *   points1/points2: all clouds concatenated, [offsets[n][t], 3] float32;  offsets: [n_examples + 1][2] row offsets
 *   (int64, start at 0, non-decreasing; an empty cloud samples as zeros like provider.py:97-98);
 *   labels: [n_examples][12] float32 = translation(3) rel_angle start_position(3) end_position(3) start_angle end_angle
 *   (the meta/<id>.json fields read at provider.py:86-89).  Host pointers; copied, not retained.
 * sample(): rows = example rows (not ids) of the batch; point n of cloud t of example r is a function of
 *   (seed, r, t, n) only.  jitter_sigma <= 0 disables the jitter (evaluation, train.py:434); clip must be > 0 otherwise.
 * batch(): device pointers of the last sampled batch (valid until the next sample()/upload()/destroy()).
 * train_step_dataset = sample + alignnet_train_step_device;  forward_dataset = sample (no jitter) + forward to host. */
int alignnet_dataset_upload(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets,
                            const float* labels, int64_t n_examples);
int alignnet_dataset_free(alignnet_handle* h);
int alignnet_dataset_sample(alignnet_handle* h, const int32_t* rows, int32_t B, uint64_t seed, float jitter_sigma,
                            float jitter_clip);
int alignnet_dataset_batch(alignnet_handle* h, const float** d_pcs1, const float** d_pcs2, alignnet_labels* d_labels);
int alignnet_train_step_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, uint64_t seed, float jitter_sigma,
                                float jitter_clip, alignnet_step_result* result);
int alignnet_forward_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, uint64_t seed, const alignnet_outputs* out);

/* ---- ICP refinement of the prediction on the full clouds -------------------------------
 * Replaces icp.icp_p2point (icp.py:69-78: o3.registration_icp, point-to-point, with_constraint=True = rotation about z
 * only, with_scaling=False) as called by the evaluation loop (train.py:463-484: radius 0.1, --its iterations,
 * init = get_mat_angle(pred_translation, pred_angle, pred_s2_pc1center), tp_utils/pointcloud.py:279-289).
 * points1 = source clouds, points2 = target clouds, concatenated; offsets [B + 1][2] as in alignnet_dataset_upload;
 * init / out: [B][16] row-major 4x4 float64 (out maps source onto target: q ~ out * p); fitness / rmse / iterations:
 * [B] each, may be NULL (Open3D's RegistrationResult fields + the number of estimate steps taken).
 * Stops like Open3D: after `its` estimates or when fitness and inlier rmse both change by < 1e-6.
 * _dataset: the clouds of the uploaded dataset (alignnet_dataset_upload) addressed by example rows -- "Careful: Pass
 * full point cloud, not subsampled one" (train.py:469). */
int alignnet_icp_refine(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                        const double* init, double radius, int32_t its, double* out, double* fitness, double* rmse,
                        int32_t* iterations);
int alignnet_icp_refine_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, double radius,
                                int32_t its, double* out, double* fitness, double* rmse, int32_t* iterations);

/* ---- ICP registration with a choice of estimate (the ICP baseline evaluation mode, icp.py:150-213) ------------
 * Same arguments and results as alignnet_icp_refine / _dataset, plus `flags`: bit 0 set = full 3-D rotation (Open3D's
 * TransformationEstimationPointToPoint with with_constraint=False: Eigen::umeyama over the inlier correspondences,
 * no scaling); clear = the z-constrained estimate, bit-identical to alignnet_icp_refine*.  Other bits are an error. */
#define ALIGNNET_ICP_FULL_ROTATION 1
int alignnet_icp_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                          const double* init, double radius, int32_t its, int32_t flags, double* out, double* fitness,
                          double* rmse, int32_t* iterations);
int alignnet_icp_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, double radius,
                                  int32_t its, int32_t flags, double* out, double* fitness, double* rmse, int32_t* iterations);
/* ---- evaluation of given transforms: what needs no ground truth (Open3D's evaluate_registration and
 * get_information_matrix_from_point_clouds; tests/reg_eval_ref.py is the definition) ---------------------------
 * Clouds as in alignnet_icp_register / _dataset (concatenated with offsets [B + 1][2], or rows of the uploaded dataset);
 * transforms [B][16] row-major 4x4 float64 (source onto target).  Per pair ONE correspondence step at its transform and
 * nothing else: the nearest target of every transformed source point by the ICP kernel's own rule (fp64 decision, equal
 * distances to the lower index), an inlier when dist2 <= threshold^2 (the closed interval of the ICP loop).
 *   fitness [B] = inliers / n1;  rmse [B] = sqrt(sum dist2 / inliers), 0 without inliers.
 *   correspondences (int32, may be NULL): per source point the chosen target's index within its cloud, -1 when not an
 *     inlier.  Host form: indexed by the offsets table's source ranges ([offsets[B][0]] entries); _dataset: the rows'
 *     source ranges back to back in `rows` order.
 *   information [B][36] (may be NULL): row-major 6x6, parameters (rotation x, y, z; translation x, y, z) = the sum over
 *     the inliers of G^T G, G = [0, z, -y, 1, 0, 0; -z, 0, x, 0, 1, 0; y, -x, 0, 0, 0, 1] for the inlier's TARGET point
 *     minus the pair's row of centers [B][3] = (x, y, z); centers NULL = the origin, Open3D's definition.  fp64 sums
 *     in a fixed order; symmetric bit for bit.
 * An empty source or target cloud: fitness 0, rmse 0, correspondences -1, a zero matrix.  The search is the handle's
 * "icp_search" option as for alignnet_icp_register.  Errors (null transforms / fitness / rmse / offsets / rows, B < 1,
 * threshold <= 0, decreasing offsets, a row out of range, no dataset) are found before anything is queued.
 * Added without moving ALIGNNET_ABI_VERSION (as alignnet_register was). */
int alignnet_evaluate_registration(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets,
                                   int32_t B, const double* transforms, double threshold, const double* centers,
                                   double* fitness, double* rmse, double* information, int32_t* correspondences);
int alignnet_evaluate_registration_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* transforms,
                                           double threshold, const double* centers, double* fitness, double* rmse,
                                           double* information, int32_t* correspondences);
/* Test hook: ONE evaluation (the correspondence step at the transform T [16], no estimate) of one pair by the kernel of
 * alignnet_icp_register* itself (the same scan source, compiled with a record behind it), and what it decided for
 * every source point: index [n1] the chosen target (-1: empty target cloud); dist2 [n1] its squared distance, fp64;
 * inlier [n1] 1 when dist2 <= radius^2; paths [n1] what the four lanes of the point's quad did with their slices of the
 * LDS-resident targets -- bits 2 s, 2 s + 1 for lane s (targets s, s + 4, ...): 0 = none (nothing under the fp32
 * certificate's threshold), 1 = single (one target decided in fp64), 2 = walk (the slice walked in fp64) -- and bit 8 set
 * when the winner came from the fp64 tail behind the LDS stage.  lds_points: 0 = as shipped (min(4266, n2)), else the
 * number of targets staged in LDS (1 .. 4266: reaches the tail with small clouds); lds_points_used [1] what was used.
 * flags as for alignnet_icp_register; fitness / rmse [1] of this evaluation, may be NULL.
 * Like every alignnet_debug_* entry this is outside the stable surface: ALIGNNET_ABI_VERSION does not move for it. */
int alignnet_debug_icp_scan(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                            const double* T, double radius, int32_t flags, int32_t lds_points, int32_t* index,
                            double* dist2, int32_t* inlier, int32_t* paths, int32_t* lds_points_used, double* fitness,
                            double* rmse);
/* The same read-back through the GRID search (alignnet_set_option "icp_search"): the grid build and ONE evaluation of one
 * pair by the shipped grid kernel's source, compiled with a record behind it.  index [n1] the chosen target's original
 * index (-1: no candidate in the 27 cells around the point); dist2 [n1] its fp64 squared distance (+inf if none; beyond
 * radius^2 it is the nearest CANDIDATE, which need not be the nearest target); inlier [n1]; candidates [n1] the
 * records evaluated for the point (a bucket met twice counts twice).  cell_edge [1] the cell edge used (> radius);
 * buckets_occupied / largest_bucket [1] of the pair's hashed cell table.  flags, fitness, rmse as above. */
int alignnet_debug_icp_grid(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                            const double* T, double radius, int32_t flags, int32_t* index, double* dist2, int32_t* inlier,
                            int32_t* candidates, double* cell_edge, int32_t* buckets_occupied, int32_t* largest_bucket,
                            double* fitness, double* rmse);

/* ---- point-to-plane ICP (the method icp.py:81-82 names and leaves `assert False`; semantics: tests/icp_plane_ref.py) --
 * Same clouds, offsets, init / out and result arrays as alignnet_icp_register.  Per pair: normals of the TARGET, once --
 * all target points within `normal_radius` (the point included, no cap), fewer than 3 give (0, 0, 1), else the unit
 * eigenvector of the smallest eigenvalue of their covariance with n_z >= 0 -- then the loop of alignnet_icp_register
 * (nearest target within `radius`, fitness / rmse of point distances, the same stop rule) with the estimate that
 * minimises sum ((U p - q) . n)^2 linearised about the pair's first target point: six unknowns with
 * ALIGNNET_ICP_FULL_ROTATION in `flags`, else rotation about z + translation (four).  A singular system (a pivot of the
 * diagonally scaled normal matrix <= 1e-10: a single plane) or no correspondence leaves the transform as it is.  Any
 * other bit of `flags` is an error.  Always the grid search: "icp_search" is not read.  The grids, normals and counts
 * live in the workspace of the grid search (alignnet_icp_free releases it). */
int alignnet_icp_plane_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets,
                                int32_t B, const double* init, double radius, double normal_radius, int32_t its,
                                int32_t flags, double* out, double* fitness, double* rmse, int32_t* iterations);
int alignnet_icp_plane_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init,
                                        double radius, double normal_radius, int32_t its, int32_t flags, double* out,
                                        double* fitness, double* rmse, int32_t* iterations);
/* Test hook: one pair through the shipped kernels' source (the loop kernel compiled with a record behind it): the normals
 * [n2][3] and neighbour counts [n2] of the target, ONE evaluation at T [16] -- index [n1] (-1: no candidate), dist2 [n1]
 * (+inf without), inlier [n1], residual [n1] = (p - q) . n of the inliers (0 otherwise) -- the reduced sums [29] (count,
 * sum of dist2, the upper triangle of J^T J row by row, J^T r; the 16 of the z-constrained estimate first, zeros behind)
 * and the update [16] (row-major 4x4) of the estimate that follows.  fitness / rmse [1] may be NULL. */
int alignnet_debug_icp_plane(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                             const double* T, double radius, double normal_radius, int32_t flags, double* normals,
                             int32_t* neighbours, int32_t* index, double* dist2, int32_t* inlier, double* residual,
                             double* sums, double* update, double* fitness, double* rmse);

/* ---- generalized (plane-to-plane) ICP (Segal, Haehnel, Thrun 2009; semantics: tests/icp_generalized_ref.py) -------------
 * Arguments, results, flags and errors of alignnet_icp_plane_register*.  Per pair, once: normals of the target AND of the
 * source, each cloud on its own by the rule above (the source's in its own frame).  A point with unit normal n has the
 * covariance C = I - (1 - 1e-3) n n^T; the loop of alignnet_icp_register with the estimate that minimises
 * sum d^T (C_q + R C_p R^T)^-1 d, d = U p - q, R = the rotation of the current transform, linearised about the pair's first
 * target point and solved as point-to-plane's system is (same scaling, same pivot floor, same update).  Motion along a
 * surface is penalised weakly instead of left free: a single plane gives a regular system.  Always the grid search.
 * Workspace per pair: point-to-plane's, a third grid over the source, its ordered records, normals and counts, one int
 * per source point. */
int alignnet_icp_generalized_register(alignnet_handle* h, const float* points1, const float* points2,
                                      const int64_t* offsets, int32_t B, const double* init, double radius,
                                      double normal_radius, int32_t its, int32_t flags, double* out, double* fitness,
                                      double* rmse, int32_t* iterations);
int alignnet_icp_generalized_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init,
                                              double radius, double normal_radius, int32_t its, int32_t flags,
                                              double* out, double* fitness, double* rmse, int32_t* iterations);
/* Test hook, as alignnet_debug_icp_plane: normals [n][3] and neighbour counts [n] of the target and of the source, ONE
 * evaluation at T [16] -- index / dist2 / inlier [n1] -- the reduced sums [29] (count, sum of dist2, the upper triangle
 * of J^T M J row by row, J^T M d; the 16 of the z-constrained estimate first, zeros behind) and the update [16]. */
int alignnet_debug_icp_generalized(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                                   const double* T, double radius, double normal_radius, int32_t flags,
                                   double* target_normals, int32_t* target_neighbours, double* source_normals,
                                   int32_t* source_neighbours, int32_t* index, double* dist2, int32_t* inlier,
                                   double* sums, double* update, double* fitness, double* rmse);

/* ---- multi-scale (coarse-to-fine) ICP (Open3D's multi_scale_icp; definition: tests/icp_multiscale_ref.py) --
 * Clouds, offsets, init / out, fitness and rmse as alignnet_icp_register.  The call has L levels, 1 <= L <= 8, described by
 * three arrays of L: voxel_sizes[l] > 0 voxel-downsamples both clouds of every pair at that edge (origin = the cloud's
 * float32 minimum per axis as a double minus half an edge, floor((p - origin) / edge) in fp64, output in ascending (ix, iy,
 * iz), the mean of a voxel's points summed in fp64 in ascending point index, divided by their number and rounded to
 * float32), <= 0 takes the raw clouds; radii[l] > 0 is the level's correspondence radius; its[l] >= 0 its iteration budget
 * (0: evaluate only).  Level l runs the ICP named by `estimate` -- 1 alignnet_icp_register, 2 alignnet_icp_plane_register,
 * 4 alignnet_icp_generalized_register, the values of alignnet_register_options.refine -- on its clouds from the transform
 * of level l - 1 (level 0: init), with normals (2, 4) taken on the level's own clouds within normal_radii[l] (> 0; may be
 * NULL for estimate 1).  flags: bit 0 = full rotation.  out / fitness / rmse are the last level's, on its clouds at its
 * radius; iterations [B][L] and level_sizes [B][L][2] (source, target points of the level) may be NULL.  The level clouds
 * and the transforms between levels stay on the device: the host waits twice, for the levels' sizes and for the results.
 * A cloud wider than 2^21 voxels on an axis at one of the voxel sizes, or with a coordinate that is not finite, fails the
 * call; so does an L out of range, a radius <= 0, a negative its or a NULL list, before anything is launched.  The
 * point-to-point levels search as "icp_search" says.  Workspace: the handle's, grown on demand ("icp_multiscale_ws_bytes"
 * reads what the last call carved): 24 bytes per raw point and downsampled level plus the tables. */
int alignnet_icp_multiscale_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets,
                                     int32_t B, const double* init, int32_t L, const double* voxel_sizes, const double* radii,
                                     const int32_t* its, const double* normal_radii, int32_t estimate, int32_t flags,
                                     double* out, double* fitness, double* rmse, int32_t* iterations, int32_t* level_sizes);
int alignnet_icp_multiscale_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const double* init, int32_t L,
                                             const double* voxel_sizes, const double* radii, const int32_t* its,
                                             const double* normal_radii, int32_t estimate, int32_t flags, double* out,
                                             double* fitness, double* rmse, int32_t* iterations, int32_t* level_sizes);
/* Test hook: the level clouds of ONE cloud of n points through the shipped pyramid kernels.  Every output holds L slots of n
 * entries; level l fills the first sizes[l] of its slot: cloud [L][n][3] the float32 points the ICP reads, means [L][n][3]
 * the fp64 means before the rounding, voxels [L][n][3] the voxel indices, counts [L][n] the points per voxel.  A level with
 * voxel <= 0 is the caller's own cloud: sizes[l] = n and its slots are left as they are. */
int alignnet_debug_voxel_pyramid(alignnet_handle* h, const float* points, int64_t n, int32_t L, const double* voxel_sizes,
                                 float* cloud, double* means, int32_t* voxels, int32_t* counts, int64_t* sizes);

/* ---- one-call registration: two raw clouds per pair in, a 4x4 transform per pair out ------------
 * The chain the evaluation loop joins in host Python (train.py:447-481), queued as one piece on the device: the
 * sampler (alignnet_dataset_sample's draw, no jitter), the eval forward, the decode of the three yaws in fp64
 * (models/tp8.py:55-65 classLogits2angle: first maximum of the nb class logits, angle = class * (2 pi / nb) +
 * residual logit of that class, minus 2 pi when > pi; the residual is not de-normalised), pred_angle = (a2 - a1) + a_rem,
 * T_net = get_mat_angle(pred_translation, pred_angle, rotation_center = pred_s2_pc1center) (evaluation.py:46-57:
 * rotation about z around the centre, then the translation; float32 inputs widened, everything else float64), and with
 * `refine` the ICP of alignnet_icp_register (1), alignnet_icp_plane_register (2) or alignnet_icp_generalized_register (4;
 * 3 is not assigned and stays an error) on the FULL clouds from T_net:
 * the handle's "icp_search" option, that entry point's stop rule and results, bit for bit what it returns for
 * init = T_net.  Nothing returns to the host between the stages: one synchronisation, at the end, with the downloads;
 * the buffers live in a workspace on the handle that grows with B (and, for host clouds, with their size) and is
 * released by alignnet_destroy.
 *   alignnet_register_dataset: rows of the uploaded dataset; draws the batch alignnet_forward_dataset(rows, B, seed)
 *     draws, so `net` receives exactly what that call returns.
 *   alignnet_register: clouds from the host, concatenated, offsets [B + 1][2] as in alignnet_icp_register.  Pair b is
 *     drawn as the dataset form would draw it were the pair installed as example streams[b] (NULL: b, the pair index).
 *   An empty cloud samples to N points at the origin (provider.py:97-98); ICP leaves such a pair at T_net.
 *   options: refine 0 = none (its must be 0; fitness / rmse / iterations must be NULL), 1 = point-to-point, 2 =
 *     point-to-plane, 4 = generalized; its >= 0; flags = ALIGNNET_ICP_FULL_ROTATION or 0; radius > 0 when refining;
 *     normal_radius > 0 for refine 2 and 4.
 *   outputs: every pointer may be NULL except transforms.  transforms / network_transforms [B][16] row-major float64
 *     (transforms = the refined estimate, or T_net without refinement); angles [B][4] = a1, a2, a_rem, pred_angle;
 *     net = host arrays for the eight raw forward outputs (each may be NULL); loss [17] = loss + the 16 summaries of
 *     alignnet_eval_loss against the dataset's labels of the rows (_dataset only; a partial batch is the caller's
 *     business).
 * Errors (null arguments, B < 1, offsets that decrease or start below 0, a row out of range, no dataset, bad option
 * values) are found before anything is queued: the engine's state is what it was. */
typedef struct {
  int32_t refine;        /* 0 none, 1 point-to-point, 2 point-to-plane, 4 generalized */
  int32_t its;           /* ICP iterations, >= 0; with refine 0 must be 0 */
  int32_t flags;         /* ALIGNNET_ICP_FULL_ROTATION or 0; anything else is an error */
  double  radius;        /* > 0 when refine != 0 */
  double  normal_radius; /* refine 2 and 4 only */
} alignnet_register_options;

typedef struct {         /* every pointer may be NULL except transforms */
  double* transforms;          /* [B][16] final estimate: refined, or T_net when refine == 0 */
  double* network_transforms;  /* [B][16] T_net */
  double* angles;              /* [B][4] a1, a2, a_rem, pred_angle (fp64) */
  const alignnet_outputs* net; /* the eight raw forward outputs, as alignnet_forward_dataset fills them */
  double* fitness; double* rmse; int32_t* iterations;  /* of the refinement; error if non-NULL with refine == 0 */
  float*  loss;                /* [17] loss + 16 summaries vs the dataset's labels; _dataset only */
} alignnet_register_outputs;

int alignnet_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets,
                      int32_t B, uint64_t seed, const int64_t* streams, const alignnet_register_options* options,
                      const alignnet_register_outputs* outputs);
int alignnet_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, uint64_t seed,
                              const alignnet_register_options* options, const alignnet_register_outputs* outputs);

/* ---- global registration: RANSAC on FPFH feature matches (the `o3_gicp` baseline, icp.py:85-143) --------------
 * Per pair: voxel downsample (0.05 m) of both clouds, normals (radius 0.10, 30 nearest), FPFH (radius 0.25, 100
 * nearest), nearest-feature matches, then RANSAC (4 correspondences, edge-length 0.9 and distance checks, threshold
 * 0.075, validated hypotheses scored by fitness then inlier rmse); no ICP follows.  Open3D is not available: the
 * computation is DEFINED by tests/global_reg_ref.py (unpinned; the downsample's output order and the random
 * generator are this project's own).  Clouds and offsets as in alignnet_icp_register; `flags` bit 0 =
 * ALIGNNET_ICP_FULL_ROTATION (Umeyama estimate), clear = rotation about z only.  `seed` and the per-pair `streams`
 * ([B] ids in [0, 2^24), NULL = all zero) select the draws: a pair's result depends on (seed, stream, clouds,
 * arguments) only, never on the batch.  max_iteration <= 2^38 and max_validation are Open3D's
 * RANSACConvergenceCriteria (4000000, 500).  out_T: [B][16] row-major 4x4 float64 (identity when nothing was
 * validated: an empty cloud, fewer than 4 downsampled points, no draw passing the checks); out_fitness / out_rmse /
 * out_iterations (iterations run) / out_validations: [B] each, may be NULL.
 * _dataset: the clouds of the uploaded dataset (alignnet_dataset_upload) addressed by example rows. */
int alignnet_global_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                             int32_t flags, uint64_t seed, const int32_t* streams, int64_t max_iteration, int32_t max_validation,
                             double* out_T, double* out_fitness, double* out_rmse, int64_t* out_iterations,
                             int32_t* out_validations);
int alignnet_global_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, int32_t flags, uint64_t seed,
                                     const int32_t* streams, int64_t max_iteration, int32_t max_validation, double* out_T,
                                     double* out_fitness, double* out_rmse, int64_t* out_iterations, int32_t* out_validations);
/* Test hook: one pair, with the stage outputs the tests pin on.  cap >= max(n1, n2) is the row stride of the per-cloud
 * arrays (index 0 = source, 1 = target): counts [2] downsampled sizes; points [2][cap][3]; voxels [2][cap][3] voxel
 * indices; voxel_points [2][cap] points per voxel; normals [2][cap][3]; spfh, fpfh [2][cap][33]; matches [cap] target
 * index of every downsampled source point; winning_iteration [1] (-1: none). */
int alignnet_debug_global_stages(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                                 int32_t flags, uint64_t seed, int32_t stream, int64_t max_iteration, int32_t max_validation,
                                 int64_t cap, int32_t* counts, double* points, int32_t* voxels, int32_t* voxel_points,
                                 double* normals, double* spfh, double* fpfh, int32_t* matches, int64_t* winning_iteration,
                                 double* out_T, double* out_fitness, double* out_rmse, int64_t* out_iterations,
                                 int32_t* out_validations);

/* ---- fast global registration (FGR) on FPFH feature matches (the `o3_gicp_fast` baseline, icp.py:121-143) ------
 * Per pair: the same downsample, normals, FPFH and nearest-feature matches as alignnet_global_register, then Open3D
 * 0.7's FastGlobalRegistration (Zhou, Park, Koltun, ECCV 2016): both clouds centred and divided by the largest
 * centred norm; matches both ways and the cross check; the tuple test (ncorr * 100 trials of three correspondences,
 * edge lengths within tuple_scale of each other, the first maximum_tuple_count passing trials kept); iteration_number
 * Gauss-Newton steps with the line-process weight (mu / (r.r + mu))^2, mu starting at 1; no ICP follows.  Open3D is
 * not available: the computation is DEFINED by tests/fgr_ref.py (unpinned; the trial draws, the order of the
 * cross-checked list, the singularity test of the solve and the z-constrained form are this project's own).
 * `flags`: bit 0 = ALIGNNET_ICP_FULL_ROTATION (six unknowns), clear = rotation about z only (x_2, t: a 4 x 4 system);
 * ALIGNNET_FGR_DECREASE_MU: after every 4th iteration (0, 4, ...), while mu > maximum_correspondence_distance,
 * mu /= division_factor.  Other bits are an error.  seed / streams as for alignnet_global_register.  Open3D's
 * option values: division_factor 1.4, maximum_correspondence_distance 0.025, iteration_number 64, tuple_scale 0.95,
 * maximum_tuple_count 1000.  Arguments outside their ranges (division_factor < 1, a distance <= 0, iteration_number or
 * maximum_tuple_count outside [0, 2^20], tuple_scale outside (0, 1]) fail; nothing is clamped.
 * out_T: [B][16] row-major 4x4 float64 mapping the source onto the target (identity for an empty cloud; the
 * translation between the downsampled means when fewer than 10 correspondences pass the tuple test); out_fitness /
 * out_rmse: inlier share and rmse of out_T on the downsampled clouds within maximum_correspondence_distance;
 * out_correspondences: correspondences the tuple test kept (3 per passing trial); out_trials: trials drawn.  [B]
 * each, may be NULL. */
#define ALIGNNET_FGR_DECREASE_MU 2
int alignnet_fgr_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                          int32_t flags, uint64_t seed, const int32_t* streams, double division_factor,
                          double maximum_correspondence_distance, int32_t iteration_number, double tuple_scale,
                          int32_t maximum_tuple_count, double* out_T, double* out_fitness, double* out_rmse,
                          int32_t* out_correspondences, int64_t* out_trials);
int alignnet_fgr_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, int32_t flags, uint64_t seed,
                                  const int32_t* streams, double division_factor, double maximum_correspondence_distance,
                                  int32_t iteration_number, double tuple_scale, int32_t maximum_tuple_count, double* out_T,
                                  double* out_fitness, double* out_rmse, int32_t* out_correspondences, int64_t* out_trials);
/* Test hook: one pair, with the stage outputs the tests pin on.  cap >= max(n1, n2) is the row stride of the per-cloud
 * arrays (index 0 = source, 1 = target): counts [4] = downsampled sizes, cross-checked pairs, accepted tuples; points
 * [2][cap][3]; fpfh [2][cap][33]; matches [cap] target index of every downsampled source point; reverse_matches [cap]
 * source index of every downsampled target point; cross [cap] source indices of the mutual matches, ascending;
 * tuple_source / tuple_target [3 maximum_tuple_count] the correspondences in trial order; tuple_trials
 * [maximum_tuple_count] the trial of every accepted tuple; normalisation [7] the two means and the scale; trace
 * [iteration_number][16] the transform after every iteration (normalised frame, target onto source). */
int alignnet_debug_fgr_stages(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                              int32_t flags, uint64_t seed, int32_t stream, double division_factor,
                              double maximum_correspondence_distance, int32_t iteration_number, double tuple_scale,
                              int32_t maximum_tuple_count, int64_t cap, int32_t* counts, double* points, double* fpfh,
                              int32_t* matches, int32_t* reverse_matches, int32_t* cross, int32_t* tuple_source,
                              int32_t* tuple_target, int64_t* tuple_trials, double* normalisation, double* trace,
                              double* out_T, double* out_fitness, double* out_rmse, int32_t* out_correspondences,
                              int64_t* out_trials);

/* ---- Go-ICP: branch-and-bound over yaw and a translation box (the `goicp` baseline, icp.py:146-147, 188-189) -----
 * The reference names the method and leaves it `assert False`; the computation is DEFINED by tests/goicp_ref.py (DESIGN.md
 * 4.7e).  Rotation about z only.  Per pair: working sets S (the source, or its points floor(i n1 / max_source)) and Q
 * (likewise, max_target), centred in fp64; T(theta, t): x -> Rz(theta)(x - mean S) + mean Q + t over theta in
 * [-yaw_half, yaw_half], t_k in [-t_half[k], t_half[k]]; E = sum_i min(d_i, trunc)^2 with d_i the distance of T(s_i) to
 * its nearest target.  A level-synchronous search halves every dimension whose half-width is above its resolution
 * (yaw_res, t_res), keeps the nodes whose lower bound is below best - mse_thresh |S|, and stops with a status:
 * CERTIFIED (no node left), RESOLUTION (only leaves left), OVERFLOW (survivors x children > max_frontier), LEVELS
 * (max_levels levels evaluated), EMPTY (a cloud without points: identity, error 0).  `starts` z-constrained point-to-point
 * ICP runs (alignnet_icp_refine's loop, radius start_radius, start_its iterations) on the working sets from yaws
 * 2 pi k / starts give the initial bound; 0 = none.  stage_points: targets staged in LDS at once, 0 = 2048 (a test hook
 * for the chunked path; a multiple of 16).  flags must be 0.
 * out_T [B][16] row-major 4x4 float64 about the origin, as the other register calls return; out_error [B] = E at the
 * returned pose; out_lower_bound [B] = min(error - mse_thresh |S|, lowest bound of the nodes still open): no pose of the
 * domain has a smaller E; out_fitness [B]; out_status [B]; out_evaluated / out_survived [B][ALIGNNET_GOICP_MAX_LEVELS] nodes per level.
 * Every pointer but out_T may be NULL.  A pair's result depends on its clouds and the parameters only.
 * _dataset: the clouds of the uploaded dataset addressed by example rows.
 * alignnet_debug_goicp_nodes (test hook, outside the stable surface): one pair, K nodes as integer coordinates
 * coords [K][4] in [0, 2^depth[k]) at the halvings depth [4] of (theta, x, y, z), through the search's own evaluation
 * kernel: ub [K] = E at the node's centre, lb [K] its lower bound.
 * (Added without moving ALIGNNET_ABI_VERSION, as alignnet_register was.) */
#define ALIGNNET_GOICP_MAX_LEVELS 24
#define ALIGNNET_GOICP_CERTIFIED 0
#define ALIGNNET_GOICP_RESOLUTION 1
#define ALIGNNET_GOICP_OVERFLOW 2
#define ALIGNNET_GOICP_LEVELS 3
#define ALIGNNET_GOICP_EMPTY 4
typedef struct {
  double yaw_half;       /* [0, pi] */
  double t_half[3];      /* >= 0; a zero-width dimension is never split */
  double yaw_res, t_res; /* > 0 */
  double trunc;          /* > 0, may be +inf */
  double mse_thresh;     /* >= 0 */
  double start_radius;   /* > 0 when starts > 0 */
  double fitness_radius; /* >= 0: out_fitness = the share of S within it at the returned pose */
  int32_t max_source, max_target;   /* [1, 2^16], [1, 2^20] */
  int32_t max_frontier;  /* [1, 2^24] nodes per pair */
  int32_t max_levels;    /* [1, ALIGNNET_GOICP_MAX_LEVELS] */
  int32_t starts;        /* [0, 64] */
  int32_t start_its;     /* >= 0 */
  int32_t stage_points;  /* 0, or a multiple of 16 in [16, 2048] */
  int32_t flags;         /* 0 */
} alignnet_goicp_params;

int alignnet_goicp_register(alignnet_handle* h, const float* points1, const float* points2, const int64_t* offsets, int32_t B,
                            const alignnet_goicp_params* params, double* out_T, double* out_error, double* out_lower_bound,
                            double* out_fitness, int32_t* out_status, int32_t* out_evaluated, int32_t* out_survived);
int alignnet_goicp_register_dataset(alignnet_handle* h, const int32_t* rows, int32_t B, const alignnet_goicp_params* params,
                                    double* out_T, double* out_error, double* out_lower_bound, double* out_fitness,
                                    int32_t* out_status, int32_t* out_evaluated, int32_t* out_survived);
int alignnet_debug_goicp_nodes(alignnet_handle* h, const float* points1, int64_t n1, const float* points2, int64_t n2,
                               const alignnet_goicp_params* params, const int32_t* depth, const int32_t* coords, int32_t K,
                               double* ub, double* lb);

/* ---- multiway registration: pose-graph optimisation of G graphs in one call (csrc/alignnet_posegraph.hip; semantics:
 * tests/pose_graph_ref.py) ----------------------------------------------------------------------------
 * Graphs are concatenated: node_offsets / edge_offsets [G + 1] (from 0, non-decreasing; a graph has >= 1 nodes), poses
 * [nodes][16] row-major 4x4 float64 (node frame -> the graph's frame; node 0 of a graph is never moved), edges [edges][2] =
 * (i, j), node numbers inside the edge's graph, i != j; transforms [edges][16] (cloud i into frame j), informations
 * [edges][36] (evaluate_registration's 6x6 about the centre, only the upper triangle is read), centres [edges][3] (frame
 * j), uncertain [edges] (0: an odometry edge; otherwise a loop closure under the line process), mu [G] > 0.
 * flags: ALIGNNET_ICP_FULL_ROTATION = six unknowns per node, otherwise yaw + translation (four).
 * One workgroup per graph runs Levenberg-Marquardt to the end on the device: at most max_solves >= 1 linear solves.
 * Nodes that no chain of edges joins to node 0 are held at their given pose, to the bit.
 * out_poses [nodes][16]; out_before / out_after [G] the objective at the given and the final poses; out_solves [G];
 * out_status [G] (ALIGNNET_POSE_GRAPH_*; EMPTY: one node, no edge or nothing to move: the given poses); out_chi2 /
 * out_weights [edges] at the final poses (weight 1 for certain edges).  Every out pointer but out_poses may be NULL.
 * Every index and every entry is checked before anything reaches the device.  A graph's result depends on the graph and
 * the arguments only: not on the other graphs of the call, not on the chunking ("pose_graph_ws_budget"), not on whether
 * its band lies in LDS or in the workspace ("pose_graph_lds_budget").
 * alignnet_debug_pose_graph_system (test hook, outside the stable surface): one graph, no step taken: r [m][d] (d = 4 or
 * 6), chi2 [m], weights [m], F, the dense H [N][N] and b [N], N = d (n - 1), from the kernel's own linearisation.
 * (Added without moving ALIGNNET_ABI_VERSION, as alignnet_register was.) */
#define ALIGNNET_POSE_GRAPH_CONVERGED 0
#define ALIGNNET_POSE_GRAPH_ITERATIONS 1
#define ALIGNNET_POSE_GRAPH_STALLED 2
#define ALIGNNET_POSE_GRAPH_EMPTY 3
int alignnet_pose_graph_optimize(alignnet_handle* h, int32_t G, const int64_t* node_offsets, const int64_t* edge_offsets,
                                 const double* poses, const int32_t* edges, const double* transforms,
                                 const double* informations, const double* centres, const int32_t* uncertain, const double* mu,
                                 int32_t flags, int32_t max_solves, double* out_poses, double* out_before, double* out_after,
                                 int32_t* out_solves, int32_t* out_status, double* out_chi2, double* out_weights);
int alignnet_debug_pose_graph_system(alignnet_handle* h, int32_t n, int32_t m, const double* poses, const int32_t* edges,
                                     const double* transforms, const double* informations, const double* centres,
                                     const int32_t* uncertain, double mu, int32_t flags, double* r, double* chi2,
                                     double* weights, double* F, double* H, double* b);

/* ---- spinning-LiDAR scene generator (the SynthCars-style datasets, tp_utils/pointcloud.py:945-971,1055-1186) -------
 * A 64 x 4500-ray sensor at the origin (ray index = row * 4500 + column, direction 120 (sin h, cos h, tan v), vfov 26.9
 * degrees, 360 degrees around) is cast against a triangle mesh at two poses per scene; the first hit of every ray is kept
 * in ascending ray index and clipped range-dependent noise is added (SyntheticScene.generate_pointcloud_embree).  trimesh
 * and embree are not available: the computation is DEFINED by tests/scene_ref.py (fp64: hit or miss and the smallest
 * t > 0 are decided in double precision; triangles are two-sided, zero-area triangles never hit).  The noise is
 * clip(strength z, +-clip) added in float32 to float32(t d), strength = max(0.005, sigma |centroid| / 80) with the
 * area-weighted centroid of the posed mesh, z standard normal from the dataset sampler's counter hash keyed by (seed,
 * scene id, cloud, ray index): a result never depends on the batch it was generated in, and it is NOT
 * np.random.randn's stream (parity unpinned by construction).
 * alignnet_scene_set_sensor: the direction tables (dir_x, dir_y [4500] = 120 sin h, 120 cos h; dir_z [64] = 120 tan v)
 *   as the caller computed them, so that device and caller cast the same rays bit for bit; without it the library's own
 *   evaluation of the same formulas is used.
 * alignnet_scene_upload_meshes: a library of M meshes: vertices [sum nv][3] (normalised as Mesh.__init__ does: bounds
 *   midpoint at 0, longest half extent 0.5), faces [sum nf][3] indices into the mesh's own vertices, offsets [M + 1][2]
 *   = first vertex / first face of every mesh, centroids [M][3] the area-weighted centroid of every (normalised) mesh.
 *   Everything is copied, nothing retained.  A face index out of range, a non-finite number or decreasing offsets fail.
 * alignnet_scene_generate: B >= 0 scenes; mesh [B] library index, scale [B] mesh_scale, poses [B][2][4] = x y z angle of
 *   the two clouds (world vertex = Rz(angle) (scale v) + position), scene_ids [B] (NULL = 0 .. B - 1) for the noise key.
 *   sigma <= 0: no noise.  The clouds stay on the device; offsets [B + 1][2] (may be NULL) receives the row offsets of
 *   the two point blobs in the layout of alignnet_dataset_upload / alignnet_icp_register.
 * alignnet_scene_read: copies the blobs of the last alignnet_scene_generate out (points1 / points2 [offsets[B][k]][3]).
 * alignnet_scene_install_dataset: makes the last result the HBM-resident dataset (device to device), labels [B][12] as
 *   for alignnet_dataset_upload; alignnet_dataset_sample, alignnet_train_step_dataset, alignnet_icp_register_dataset,
 *   alignnet_global_register_dataset and alignnet_fgr_register_dataset then work on it.
 * alignnet_debug_scene_cast (test hook, outside the stable surface): ONE cloud (pose [4]) by the shipped cast kernel
 *   with a record behind it, no noise: t [288000] per ray index (inf = miss), triangle [288000] the face hit (-1),
 *   window [2] = first column and number of columns of the azimuth window that was cast (it may wrap 4499 -> 0),
 *   lds_triangles: triangles per LDS chunk, 0 = as shipped (512), 1 .. 512 forces several chunks on small meshes;
 *   lds_triangles_used [1].  It discards the result of an earlier alignnet_scene_generate.  It always runs the scan.
 * alignnet_debug_scene_cast_binned (test hook, outside the stable surface): the same read-back through the BINNED cast
 *   (alignnet_set_option "scene_cast"), whatever the option says; the same arguments and lds_triangles range, and
 *   tile_counts [563] the length of the triangle list of every 8-column tile of the window (0 beyond the window's
 *   tiles), entries [1] their sum.
 * alignnet_debug_scene_cast_rows (test hook, outside the stable surface): the same read-back with the inner loop BY
 *   ELEVATION BAND (alignnet_set_option "scene_rows"), whatever the options say: binned = 0 the scan's staging, 1 the
 *   tile lists'; window, t, triangle and lds_triangles_used as above; cell_counts [563][8] the staged triangles per
 *   (8-column tile of the window, band of 8 rows) whose band bit was set (0 beyond the window's tiles), cells [1] their
 *   sum. */
int alignnet_scene_set_sensor(alignnet_handle* h, const double* dir_x, const double* dir_y, const double* dir_z);
int alignnet_scene_upload_meshes(alignnet_handle* h, const double* vertices, const int32_t* faces, const int64_t* offsets,
                                 const double* centroids, int32_t M);
int alignnet_scene_free_meshes(alignnet_handle* h);
int alignnet_scene_generate(alignnet_handle* h, const int32_t* mesh, const double* scale, const double* poses,
                            const int64_t* scene_ids, int32_t B, uint64_t seed, double sigma, double clip, int64_t* offsets);
int alignnet_scene_read(alignnet_handle* h, float* points1, float* points2);
int alignnet_scene_install_dataset(alignnet_handle* h, const float* labels);
int alignnet_debug_scene_cast(alignnet_handle* h, int32_t mesh, double scale, const double* pose, int32_t lds_triangles,
                              double* t, int32_t* triangle, int32_t* window, int32_t* lds_triangles_used);
int alignnet_debug_scene_cast_binned(alignnet_handle* h, int32_t mesh, double scale, const double* pose,
                                     int32_t lds_triangles, double* t, int32_t* triangle, int32_t* window,
                                     int32_t* lds_triangles_used, int32_t* tile_counts, int64_t* entries);
int alignnet_debug_scene_cast_rows(alignnet_handle* h, int32_t mesh, double scale, const double* pose,
                                   int32_t lds_triangles, int32_t binned, int32_t* window, double* t, int32_t* triangle,
                                   int32_t* lds_triangles_used, int32_t* cell_counts, int64_t* cells);

/* ---- KITTI tracklet extraction (the KITTITracklets* datasets, tp_utils/pointcloud.py:769-778, 840-869, 918-940, 1000-1033) ----
 * The points of a LiDAR scan inside a tracked 3D box, in scan order: extract_pointcloud -> compute_box_3d -> in_hull
 * (scipy's Delaunay.find_simplex on the eight corners) as one pass over points x boxes on the device.  The computation is
 * DEFINED by tests/tracklet_ref.py (fp64):
 *   a point p = (x, y, z) float32 in the Velodyne frame has camera-frame coordinates q = (-y, -z, x) (the reference's
 *   R = R1 R2, a signed permutation: exact); a box is b = (bx, by, bz, h, w, l, ry), the KITTI label's location, dimensions
 *   and rotation_y; d = q - (bx, by, bz) in fp64; c = cos ry and s = sin ry are evaluated once on the host in fp64;
 *   lx = c dx - s dz, ly = dy, lz = s dx + c dz, every product and difference rounded as written (no fused multiply-add);
 *   the point is inside iff |lx| <= l / 2, -h <= ly <= 0 and |lz| <= w / 2.  The box is CLOSED: a point on a face, an
 *   edge or a corner is inside.  This is the convex hull of compute_box_3d's corners (checked against scipy on the CPU:
 *   tests/test_tracklet_cpu.py).  A point with a non-finite coordinate is in no box.
 *   ORDER: a crop holds its points in scan order (the reference's pc[inds]) with their float32 bits unchanged.
 *   dz: subtracted from z in ONE float32 subtraction, z' = z (-) dz -- the reference's `pc2[:, 2] -= z_difference` on a
 *   float32 array, where the NumPy of the reference's time casts the float64 scalar to float32 before it subtracts; the
 *   caller passes float32(z_difference) for cloud 2 and 0 for cloud 1 (x - 0 keeps every bit, -0 included).
 *   No colour columns: the reference reads [:, :3] everywhere, and colours need the camera images.
 * alignnet_tracklet_upload_scans: F >= 0 frames, points [offsets[F]][stride] with stride 3 or 4 floats per point (a KITTI
 *   .bin is 4: x y z reflectance; only x y z are read), offsets [F + 1] the first point of every frame (offsets[0] = 0).
 *   Copied to the device once, nothing retained; replaces an earlier upload.  A bad stride or decreasing offsets fail and
 *   leave the earlier upload in place.
 * alignnet_tracklet_free_scans: frees the uploaded scans (the last result stays readable).
 * alignnet_tracklet_extract: B >= 0 pairs; frames [B][2] the frame index of each cloud, boxes [B][2][7] fp64 as above,
 *   dz [B][2] float32.  The two point blobs stay on the device; offsets [B + 1][2] (may be NULL) receives their row offsets
 *   in the layout of alignnet_dataset_upload / alignnet_scene_generate.  A pair's crops do not depend on what else is in
 *   the call.  A frame index out of range, a non-finite box value or dz, or a negative extent fails; a failed call leaves
 *   the previous result and the uploaded scans as they were.
 * alignnet_tracklet_read: copies the blobs of the last alignnet_tracklet_extract out (points1 / points2 [offsets[B][k]][3]).
 * alignnet_tracklet_install_dataset: makes the last result the HBM-resident dataset (device to device), labels [B][12] as
 *   for alignnet_dataset_upload; every *_dataset / *_rows entry point then works on the crops. */
int alignnet_tracklet_upload_scans(alignnet_handle* h, const float* points, int32_t stride, const int64_t* offsets, int32_t F);
int alignnet_tracklet_free_scans(alignnet_handle* h);
int alignnet_tracklet_extract(alignnet_handle* h, const int32_t* frames, const double* boxes, const float* dz, int32_t B,
                              int64_t* offsets);
int alignnet_tracklet_read(alignnet_handle* h, float* points1, float* points2);
int alignnet_tracklet_install_dataset(alignnet_handle* h, const float* labels);

/* ---- the image-frustum crop (extract_pointcloud with from_bbox2d: extract_pc_in_box2d -> get_lidar_in_image_fov ->
 * Calibration.project_velo_to_image, tp_utils/pointcloud.py:781-801, 41-202) ----
 * Every LiDAR return of an uploaded scan whose image projection falls inside an object's 2D box: the crop a tracker has before
 * any 3D box exists (a detector's rectangle plus the calibration).  DEFINED by tests/frustum_ref.py (fp64):
 *   a frame has a projection M [3][4] = P (R0 padded to 4 x 4) (V2C padded to 4 x 4), multiplied ONCE by the caller in fp64
 *   (alignnet3d.tracklets.projection), and an image size (W, H); a point p = (x, y, z) float32, widened to fp64, has
 *   w_i = ((M[i][0] x + M[i][1] y) + M[i][2] z) + M[i][3], every product and sum rounded as written (no fused multiply-add),
 *   and u = w_0 / w_2, v = w_1 / w_2 (IEEE fp64 divisions).  A job's rectangle (xmin, ymin, xmax, ymax) keeps the point iff its
 *   coordinates are finite, x > clip (the reference's clip_distance, 2.0), 0 <= u < W, 0 <= v < H, xmin <= u < xmax and
 *   ymin <= v < ymax.  The intervals are HALF-OPEN, the reference's.  A comparison with a NaN or infinite u / v is false, so a
 *   point with w_2 == 0 is in no crop; the sign of w_2 is not tested (the reference's front test is x > clip).
 *   Order, bits and dz: as for alignnet_tracklet_extract.  No colour columns.
 * alignnet_tracklet_extract_frustum: B >= 0 pairs; frames [B][2] and dz [B][2] as for alignnet_tracklet_extract; rects [B][2][4]
 *   fp64 = xmin ymin xmax ymax; proj [F][12] (M row-major) and image [F][2] = W, H for EVERY uploaded frame (F of
 *   alignnet_tracklet_upload_scans); clip one value for the call.  The result replaces, and is read and installed like, a box
 *   extraction's (alignnet_tracklet_read, alignnet_tracklet_install_dataset).  No scans uploaded, a frame index out of range, a
 *   non-finite rect, proj, image, clip or dz value, W or H <= 0 or a null argument fail before any device work and leave the
 *   previous result and the uploaded scans as they were.  xmin >= xmax or ymin >= ymax is no error: an empty crop.
 *   (Added without moving ALIGNNET_ABI_VERSION, as alignnet_register was.) */
int alignnet_tracklet_extract_frustum(alignnet_handle* h, const int32_t* frames, const double* rects, const float* dz, int32_t B,
                                      const double* proj, const double* image, double clip, int64_t* offsets);

/* ---- run-time options with no counterpart in the reference's config surface --------
 * "train_matmul_bf16" (0/1, default 0): training only -- the two MFMA convs of every backbone (the hidden 1x1 conv
 *   and the -> C3 feature lift, 96 % of the step's FLOPs, models/tp8.py:55-57), in the forward and in the backward's
 *   recompute, run on bf16 MFMA with fp32 accumulation (BASELINE.json configs[2]); statistics, pooling, the K = 3 lift,
 *   the heads, gradient accumulation, optimiser state and the eval-mode forward stay fp32.  Backbones outside the fused shape: only
 *   the last conv, when it runs as the fused tail ("train_fused_tail").  With the dgcnn backbone: the edge
 *   conv behind the K = 6 lift and the point conv (forward), and the dense product h1 Q2 of the backward edge pass.
 * "train_fused_tail" (0/1, default 1): training of backbones outside the fused kernels' shape (depth != 3, odd widths; e.g. the
 *   five-layer backbones of configs/default.json): the layers up to the second-to-last run layer by layer, their output is kept once,
 *   and the last layer -- 90 % of such a backbone's FLOPs -- runs on the fused phase-3 / pass-B2 kernels on the stored features
 *   (when the last two widths fit: multiples of 32, <= 128 and <= 1024), so that the [B N, C_last] tensors never exist.  0 = every
 *   layer layer by layer.  Same arithmetic up to summation order.
 * "infer_matmul_bf16x3" (0/1, default 0): eval-mode forward of 3-layer PointNet backbones (every shipped config) -- every
 *   fp32 operand of the two MFMA layers is written x = bf16(x) + bf16(x - bf16(x)) and each product is formed as
 *   x_hi w_hi + x_hi w_lo + x_lo w_hi with fp32 accumulation: three bf16 MFMAs instead of one fp32 MFMA (16x slower on
 *   gfx950).  Outputs stay within the 1e-4 parity bar (measured 3e-6 against the fp64 oracle, like the exact path).
 *   Also covers the DGCNN branch with widths [<= 64, <= 128, C3]; other backbone shapes keep the exact-fp32 kernels.
 * "allreduce_overlap" (0/1, default 1): data-parallel training steps (alignnet_train_step*, communicator initialised) all-reduce the
 *   gradient in three buckets on a side stream -- the stage-3, stage-2 and stage-1 segment of the flat gradient.  A stage's deferred
 *   weight-gradient jobs are flushed right behind that stage's backward, its bucket is issued at once and travels under the next stage's
 *   backward, so that only the last (smallest, 14 % of the vector for the shipped widths) bucket is exposed; 0 = one all-reduce of the
 *   whole vector after the backward.  Same sums either way.  (Without a communicator the three stages' jobs stay one group of five
 *   launches after the whole backward.)
 * "train_dw_side_stream" (0/1, default 0): the weight-gradient jobs only the optimiser waits for are queued per stage on a second stream
 *   (under the next stage's backward; data-parallel: that stage's all-reduce bucket leaves right behind them) instead of as one group
 *   after the whole backward.  Same arithmetic, same summation order.  Slower on one GPU (measured).
 * "train_phase3_tile64" (0/1, default 0): the training forward's last conv layer + max-pool (phase 3) of the shipped widths 64 / 128 on
 *   64-point tiles, two workgroups per CU (rounds 1 - 2) instead of 128-point tiles, one workgroup of eight waves per CU
 *   (csrc/kernels_train_fwd_wide.h: a weight fragment of the lift feeds four row tiles instead of two).  Same lift values bit for bit; the
 *   column sums of h2 are grouped differently.  A/B switch and test hook.
 * "sync_bn" (0/1, default 0): data-parallel training with the reference's single-device BatchNorm semantics at the GLOBAL batch
 *   (utils/tf_util.py:474): every batch sum behind a BatchNorm -- forward moments, the Gram / column-sum matrices of the layer
 *   identities, the backward's (dbeta, dgamma) totals, the heads' row statistics -- is all-reduced over the ranks (RCCL, about thirty
 *   small all-reduces per step) between the kernel that forms this rank's sum and the one that uses it.  Every backbone shape: fused
 *   three-layer stages, the dgcnn branch, and stages that train layer by layer (any depth / widths: two all-reduces per layer forward --
 *   the sum, then the squared differences from the global mean -- and one backward).  0: every rank normalises with its own shard's
 *   statistics ("local BN").
 * "global_loss" (0/1, default 0): the loss and its gradient over the global batch -- the [B, B] broadcast terms (models/tp8.py:279,327)
 *   and the whole-batch tf.cond (:288) couple all samples: end points and labels are all-gathered, every rank evaluates the same
 *   global loss and keeps its rows of the gradient; the gradient all-reduce then sums instead of averaging.  With "sync_bn" a
 *   data-parallel step is the reference's step at batch B x ranks.
 * "sync_bn_emulate_world" (test hook, default 1): without a communicator, stand for this many ranks holding identical shards.
 * "dropout_stream" (default 0): selects one of 2^64 independent device-side dropout streams under the same cfg.seed; data-parallel
 *   ranks set it to their rank so that they do not draw identical masks for their local rows (initialisation stays cfg.seed's).
 * "icp_search" (0/1/2, default 0): the correspondence search of alignnet_icp_refine, _refine_dataset, _register and _register_dataset.
 *   0 = the brute-force scan for every pair (n1 x n2 distances per iteration; built for clouds of a few thousand points, and every result
 *   bit for bit what it was before the key existed).  1 = a uniform-grid search for every pair: per call the pair's targets are bucket-sorted
 *   by hashed cell (cells just over one radius wide, O(n2) memory whatever the extent), and every source point evaluates in fp64 only the
 *   targets in the 27 cells around it -- exact: the same nearest target within the radius, equal distances to the lower index; the sums run
 *   over another assignment of points to threads, so transforms agree with the scan's to rounding (1e-9), not bit for bit.  2 = automatic:
 *   a pair takes the grid when its target has more than 4266 points (where the scan leaves its LDS stage), else the scan; each pair's
 *   result is bit-identical to what 0 (scan pairs) or 1 (grid pairs) gives it.  Other values are an error.
 * "scene_cast" (0/1/2, default 0): how alignnet_scene_generate casts a cloud.  0 = the scan: every 8-column tile of the cloud's azimuth
 *   window poses and side-tests all triangles of the mesh (built for meshes of some hundred triangles; every result bit for bit what it
 *   was before the key existed).  1 = binned, for every cloud: the triangles are first binned to the tiles their azimuth interval
 *   reaches (conservative: the rule that chooses the window), and a tile poses and intersects only its own list (4 bytes per list entry,
 *   freed with the handle) -- exact: offsets and points are bit for bit the scan's.  2 = automatic: a cloud is binned when its mesh has
 *   more than 512 triangles (where the scan stops fitting the mesh in one LDS chunk), else scanned.  A cloud's result does not depend on
 *   the option or on what else is in the call.  Other values are an error.  Measured on an MI355X the scan is the faster one at every mesh
 *   size tried, 516 to 100,002 triangles (profiles/scene_cast_rate.json): 1 and 2 are exact alternatives, not accelerations, today.
 *   "scene_binned_clouds" (read-only): how many clouds of the last alignnet_scene_generate took the binned cast;
 *   "scene_bin_entries" (read-only): the entries of their tile lists together.
 * "scene_rows" (0/1, default 0): how both casts of "scene_cast" run their inner loop.  0 = every staged triangle against all 64 rows x 8
 *   columns of the tile (the kernels as they were before the key existed).  1 = by elevation band: a staged triangle carries a mask of the
 *   eight bands of 8 rows it can reach (conservative: csrc/alignnet_scene.hip, stage 2c) and is intersected only with those -- exact:
 *   offsets and points are bit for bit those of 0.  Orthogonal to "scene_cast".  Other values are an error and leave the value as it was.
 *   Measured on an MI355X (profiles/scene_rows_rate.json; README, "cast by elevation band") 1 is ahead of 0 at every mesh size tried, under
 *   both stagings: 1.57 x for a 516-triangle mesh with "scene_cast" 0, and 2.1 x - 2.7 x from 5,001 to 100,002 triangles with "scene_cast" 1,
 *   which is the faster staging there once the bands have cut the intersections.  Off by default.
 *   "icp_grid_ws_bytes" (read-only): the workspace the last call with grid pairs carved (per chunk of pairs, at most 1 GiB unless one pair
 *   needs more; freed with the handle).
 *   "icp_multiscale_ws_bytes" (read-only): the workspace the last alignnet_icp_multiscale_register* / alignnet_debug_voxel_pyramid call
 *   carved (sort records, level clouds, tables, chained results; freed with the handle).
 * "icp_plane_ws_budget" (bytes, default 0 = 1 GiB): the workspace one chunk of pairs of alignnet_icp_plane_register* may take (two grids,
 *   ordered records, normals and counts per pair; a pair that needs more forms a chunk alone).  Results do not depend on it: a smaller value
 *   only cuts a call into more chunks (a test hook for the chunking, and a way to bound the allocation).
 *   "icp_plane_chunks" (read-only): the chunks the last point-to-plane call ran.
 * "icp_generalized_ws_budget" / "icp_generalized_chunks" (read-only): the same two for alignnet_icp_generalized_register* (its pairs also hold the
 *   source's grid, ordered records, normals, counts and correspondences).
 * "pose_graph_ws_budget" (bytes, default 0 = 1 GiB) / "pose_graph_chunks" (read-only): the same two for alignnet_pose_graph_optimize (per graph:
 *   trial poses, 25 doubles per edge, and both bands, b and x when they do not lie in LDS); one launch per chunk.
 *   "pose_graph_lds_budget" (doubles, default -1 = 20000, at most 20000): a graph whose two bands, b and x (2 N (bw + 1) + 2 N doubles) fit
 *   keeps them in LDS, any other in its slice of the workspace; 0 puts every graph's in the workspace.  Results do not depend on it.
 *   "pose_graph_lds_graphs" (read-only): the graphs of the last call that took the LDS placement.
 * "tracklet_chunk" (read-only): the points of a frame one workgroup of alignnet_tracklet_extract takes (1024);
 *   "tracklet_jobs_per_pass" (read-only): the crop jobs of a frame it stages in LDS per pass (32).  Tests size their edge cases from them.
 * "ab_*" (0/1, default 0): A/B dispatch overrides -- each selects an earlier kernel variant of the SAME arithmetic for same-box comparisons
 *   (results agree up to summation order; tests/test_train_gpu.py runs them against the default): "ab_no_ld_const", "ab_infer_tile64",
 *   "ab_phase2_legacy", "ab_b1_legacy", "ab_b1_fp32", "ab_p3_bf16_generic", "ab_p3_nogram", "ab_no_defer", "ab_dg_sparse",
 *   "ab_no_glue_fold", "ab_gemm_jobs_ksplit", "ab_fc_direct", "ab_fc_no_splitk", "ab_split_tilewise", "ab_last_layer_stream" (csrc/engine.h: AbBit), and "ab_tiles_per_wg" (eval PointNet backbone: point tiles per workgroup, 0 = automatic);
 *   "dg_cloud_parts" (dgcnn training: workgroups per cloud of the edge kernels, 0 = as many as fill the chip at this batch, 1 .. 8 = fixed; results agree up to the grouping of partial sums);
 *   "infer_tile_points" (eval PointNet backbone: points per workgroup tile; 0 = automatic -- 64-point tiles while the 128-point tiling would cover at most half of the
 *   256 CUs (2B x ceil(N / 128) <= 128: B <= 8 at N = 1024; 0.19 -> 0.134 ms per step at B = 1, 0.198 -> 0.142 at B = 8), 128 otherwise; 64 / 128 = fixed; bit-identical outputs);
 *   "infer_wg_waves" (eval PointNet backbone, shipped shape on 128-point tiles: waves per workgroup; 8 = pointnet_fused<128, 68, 132, 16>, one workgroup per CU;
 *   4 = pointnet_fused_duo<128, 132, 16>, two independent workgroups per CU, one's prologue under the other's last layer; 0 = automatic -- 4 once the grid has
 *   two workgroups for every CU, 8 below; other shapes, "ab_last_layer_stream" and 64-point tiles run eight waves whatever it says; bit-identical outputs);
 *   "pn_cloud_parts" (the same split for the per-cloud kernels both backbones share: phase 2 / the first-layer Gram, phase 3 -- the lift to C3 with its running
 *   arg-extreme and Gram, the parts' extremes folded exactly in tile order -- and passes B2, B1; the chip is full from 2B = 256 (128-point-tile kernels) or 512
 *   clouds, the reference's shipped batch of 128 brings 256; 0 = automatic, 1 .. 8 = fixed).
 *   "ab_mask" (read-only) = the bits that are set; bench.py prints it.  The library reads NO environment variable; result-changing
 *   ablation switches exist only in the separate ablation build (csrc/ablate.h, `make ablate`).
 * Read-only keys (alignnet_get_option; parity tests use them to assert which kernel instantiation ran, since the shipped
 * widths 64 / 128 dispatch to kernels with the widths compiled in):
 * "last_backbone_kernel": ALIGNNET_KERNEL_* of the most recent eval-mode backbone launch (the four- and the eight-wave form of the shipped shape
 *   report the same number);  "last_backbone_wg_waves": the waves per workgroup of that launch;  "backbone_wgs_per_cu": what
 *   hipOccupancyMaxActiveBlocksPerMultiprocessor answers for its kernel, block size and dynamic LDS (PointNet fp32 kernels; 0 otherwise);
 * "comm_world": number of ranks of the communicator (0 = none); "comm_buckets": bucket all-reduces the last step issued;
 * "sync_collectives": sync_bn / global_loss collectives (per-layer all-reduces, gathers) the last training step issued;
 * "comm_order": issue order of the last training step's backward, one decimal digit per event: 1..3 = backward of stage 1..3 queued,
 *   4..6 = all-reduce bucket of stage 1..3 issued (data-parallel step with "allreduce_overlap": 362514 -- every bucket leaves before the
 *   next stage's backward is queued);
 * "last_train_kernel": bit mask of the most recent training step -- 1 = compile-time widths (64, 128), 2 = bf16 operands,
 *   4 = dgcnn backbone, 8 = at least one stage ran the general-depth (layer-by-layer) path, 16 = with its last layer on the fused
 *   kernels ("train_fused_tail").
 * Unknown keys fail. */
#define ALIGNNET_KERNEL_POINTNET_FUSED 1            /* pointnet_fused<128>: run-time widths */
#define ALIGNNET_KERNEL_POINTNET_FUSED_64_128 2     /* pointnet_fused<128, 68, 132> */
#define ALIGNNET_KERNEL_POINTNET_FUSED_64_128_K16 3 /* pointnet_fused<128, 68, 132, 16>: the shipped 3-layer shape */
#define ALIGNNET_KERNEL_POINTNET_FUSED_TP64 4       /* pointnet_fused<64> (ALIGNNET_TILE=64) */
#define ALIGNNET_KERNEL_POINTNET_FUSED_64_128_K16_TP64 8 /* pointnet_fused<64, 68, 132, 16>: the shipped shape on 64-point tiles (small batches: "infer_tile_points") */
#define ALIGNNET_KERNEL_POINTNET_SPLIT 5            /* pointnet_split<> */
#define ALIGNNET_KERNEL_POINTNET_SPLIT_64_128 6     /* pointnet_split<64, 128> */
#define ALIGNNET_KERNEL_POINTNET_SPLIT_PERSIST 7    /* pointnet_split_persist: shipped widths, persistent workgroups */
#define ALIGNNET_KERNEL_DGCNN_FUSED 10              /* dgcnn_fused<> */
#define ALIGNNET_KERNEL_DGCNN_FUSED_64_128 11       /* dgcnn_fused<68, 132> */
#define ALIGNNET_KERNEL_DGCNN_SPLIT 12              /* dgcnn_split<> */
#define ALIGNNET_KERNEL_DGCNN_SPLIT_64_128 13       /* dgcnn_split<64, 128> */
int alignnet_set_option(alignnet_handle* h, const char* key, int64_t value);
int alignnet_get_option(alignnet_handle* h, const char* key, int64_t* value);
int alignnet_profile_read(alignnet_handle* h, double* backbone_ms, int64_t* backbone_launches,
                          double* total_ms, int32_t reset);
/* HIP-event time (ms, summed) and launch count of one timed kernel since the last reset (alignnet_profile_read(..., reset = 1)), measured
 * on the stream it is launched on while profiling is enabled.  name: "backbone" (eval-mode fused backbone), "knn",
 * "train_fwd_phase2", "train_fwd_phase3", "train_gram_h2", "train_bwd_b2", "train_bwd_b1", "dg_train_fwd", "dg_train_bwd_edge",
 * "allreduce" (what the compute stream waits for), "optimizer", and the stages of alignnet_scene_generate: "scene_window" (azimuth windows),
 * "scene_cast" ("scene_band" instead when "scene_rows" is 1), "scene_compact" (counts, scan, scatter + noise), and of the ICP grid search: "icp_grid_build", "icp_grid" (the iterations), and of
 * point-to-plane ICP: "icp_plane_normals" (the ordering of the second grid's buckets + the normals), "icp_plane" (the iterations; its two grid builds
 * count under "icp_grid_build"), of generalized ICP: "icp_generalized_normals" (both clouds' orderings + normals), "icp_generalized" (the iterations; its
 * three grid builds count under "icp_grid_build"), and of alignnet_tracklet_extract and alignnet_tracklet_extract_frustum: "tracklet_test" (membership + counts), "tracklet_compact" (scan + scatter),
 * and of alignnet_pose_graph_optimize: "pose_graph" (one launch per chunk of graphs). */
int alignnet_profile_read_kernel(alignnet_handle* h, const char* name, double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNNET_HIP_H */
