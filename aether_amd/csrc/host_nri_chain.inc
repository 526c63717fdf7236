// Host side of the C ABI: the NRI chain that the models of both step engines share -- the seq2seq job-table engine
// (host_s2s_step.inc, host_s2s_dnri.inc) and the variable-N scene engine (host_dyn_dnri.inc) -- each piece once, as a plain
// function over a small struct of pointers and sizes (DESIGN 4.7d).  Null means "none" throughout (an image, a layer's BatchNorm
// scale / shift, the fused cell's bias, a decoder state); a callable stands only where a caller puts its own jobs or kernel into
// the sequence.  No checks, no layouts: those are the entries'.  Included by aether_hip.hip in front of host_seq2seq.inc.
namespace {
// (defined in host_seq2seq.inc)
int s2s_linear(int act, const float* W, int ldw, const float* b, const float* X, float* Y, int M, int K, int64_t N,
               int ldy, const float* scale, int sstride, int accumulate, hipStream_t st,
               const int64_t* xidx = nullptr, const int64_t* yidx = nullptr, const int* n_dev = nullptr,
               const float* post_scale = nullptr, const float* post_shift = nullptr,
               const float* film_gamma = nullptr, const float* film_beta = nullptr, int film_rows = 1);
// (defined in host_s2s_step.inc)
int s2s_launch_jobs(S2SJobs& T, hipStream_t st);
bool s2s_jobs_take_split(const S2SJobs& T);
S2SJob s2s_job(int act, const float* W, int ldw, const float* b, const float* X, int ldx, float* Y, int ldy, int M, int K, int64_t N);
extern "C++" dim3 nri_blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// Pointers into a step's workspace and into its plan of prepared weights (images: null where the layout has none, offset 0)
struct NriMem {
    char* ws; const char* plan;
    float* wp(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    const float* pl(size_t off) const { return reinterpret_cast<const float*>(plan + off); }
    const void* im(size_t off) const { return off ? reinterpret_cast<const void*>(plan + off) : nullptr; }
};

// A job with its weight image and the BatchNorm affine behind it; nri_one: in a launch of its own
S2SJob nri_with(S2SJob J, const void* image, const float* bn_scale = nullptr, const float* bn_shift = nullptr) {
    J.Wimg = image; J.post_scale = bn_scale; J.post_shift = bn_shift;
    return J;
}
int nri_one(hipStream_t st, S2SJob J, const void* image, const float* bn_scale = nullptr, const float* bn_shift = nullptr) {
    S2SJobs T;
    T.n = 1; T.j[0] = nri_with(J, image, bn_scale, bn_shift);
    return s2s_launch_jobs(T, st);
}

// ---- 1. mlp4 on [x_send | x_recv | third]: the node halves of the first Linear in one launch, the edge third with the two
// gathers in its epilogue, the second Linear with BatchNorm.  x_node [Nn][h], x_edge [E][h] -> out [E][h]; Ps, Pr, T: scratch
struct NriMlp4 {
    const float *w0, *b0, *w3, *b3, *bn_scale, *bn_shift;
    const void *img_ps, *img_pr, *img_edge, *img_w3;
    const float *x_node, *x_edge;
    const int64_t *send, *recv;
    float *Ps, *Pr, *T, *out;
    int h; int64_t Nn, E;
};
int nri_edge_mlp4(const NriMlp4& m, hipStream_t st) {
    const int h = m.h;
    S2SJobs T;
    T.n = 0;
    T.j[T.n++] = nri_with(s2s_job(0, m.w0, 3 * h, m.b0, m.x_node, h, m.Ps, h, h, h, m.Nn), m.img_ps);
    T.j[T.n++] = nri_with(s2s_job(0, m.w0 + h, 3 * h, nullptr, m.x_node, h, m.Pr, h, h, h, m.Nn), m.img_pr);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    S2SJob J = s2s_job(4, m.w0 + 2 * h, 3 * h, nullptr, m.x_edge, h, m.T, h, h, h, m.E);
    J.g1 = m.Ps; J.i1 = m.send; J.g2 = m.Pr; J.i2 = m.recv;
    if (int rc = nri_one(st, J, m.img_edge)) return rc;
    return nri_one(st, s2s_job(4, m.w3, h, m.b3, m.T, h, m.out, h, h, h, m.E), m.img_w3, m.bn_scale, m.bn_shift);
}

// ---- 2. one LSTM step per edge and prior_fc_out, as job tables.  [W_ih | W_hh] . [x | h0] is one job.  Where its table goes
// to the split GEMM (s2s_jobs_take_split) the cell update is the GEMM's epilogue (S2SJob act 5: the images' rows and bias_fused
// are the gates interleaved by unit -- one launch, no [E][4R] round trip); otherwise the job drops its images, which fit the
// fused form only, and k_s2s_lstm_cell follows the fp32 job kernel.  Then the 1 .. 4 head layers through Y1 / Y2 into logits
struct NriLstmHead {
    const float *w_ih, *w_hh, *bias, *bias_fused;
    const void *img_ih, *img_hh;
    const float* const* prior_w; const float* const* prior_b;
    const void* img_prior[4];
    const float *x, *h0, *c0;
    float *G, *h1, *c1, *Y1, *Y2, *logits;
    int h, R, prior_layers, ph, K; int64_t E;
};
int nri_lstm_head(const NriLstmHead& a, hipStream_t st) {
    const int R = a.R;
    const int64_t E = a.E;
    S2SJobs T;
    S2SJob J = s2s_job(0, a.w_ih, a.h, a.bias, a.x, a.h, a.G, 4 * R, 4 * R, a.h, E);
    J.W2 = a.w_hh; J.X2 = a.h0; J.K2 = R; J.ldw2 = R; J.ldx2 = R; J.Wimg = a.img_ih; J.W2img = a.img_hh;
    T.n = 0; T.j[T.n++] = J;
    if (a.bias_fused && s2s_jobs_take_split(T)) {
        T.j[0].act = 5; T.j[0].bias = a.bias_fused; T.j[0].cell_c0 = a.c0; T.j[0].cell_h1 = a.h1; T.j[0].cell_c1 = a.c1;
        if (int rc = s2s_launch_jobs(T, st)) return rc;
    } else {
        T.j[0].Wimg = nullptr; T.j[0].W2img = nullptr;
        if (int rc = s2s_launch_jobs(T, st)) return rc;
        k_s2s_lstm_cell<<<nri_blocks(E * R), dim3(256), 0, st>>>(a.G, a.c0, a.h1, a.c1, R, E);
    }
    const float* cur = a.h1;
    int cur_k = R;
    for (int l = 0; l < a.prior_layers; ++l) {
        const bool last = l + 1 == a.prior_layers;
        float* dst = last ? a.logits : l % 2 == 0 ? a.Y1 : a.Y2;
        const int M = last ? a.K : a.ph;
        if (int rc = nri_one(st, s2s_job(last ? 0 : 4, a.prior_w[l], cur_k, a.prior_b[l], cur, cur_k, dst, M, M, cur_k, E),
                             last ? nullptr : a.img_prior[l])) return rc;
        cur = dst;
        cur_k = M;
    }
    return AETHER_OK;
}

// ---- 3. the same in the older two-launch form on s2s_linear (the staged prior steps, aether_s2s_lstm_step / _mlp_head):
// W_ih . x, then W_hh . h0 accumulated into gates [rows][4R], then the cell
int nri_lstm_two_launch(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int in_size, int R,
                        int64_t rows, const float* x, const float* h0, const float* c0, float* gates, float* h1, float* c1,
                        hipStream_t st) {
    if (s2s_linear(0, w_ih, in_size, b_ih, x, gates, 4 * R, in_size, rows, 4 * R, nullptr, 0, 0, st)) return AETHER_EINVAL;
    if (s2s_linear(0, w_hh, R, b_hh, h0, gates, 4 * R, R, rows, 4 * R, nullptr, 0, 1, st)) return AETHER_EINVAL;
    k_s2s_lstm_cell<<<nri_blocks(rows * R), dim3(256), 0, st>>>(gates, c0, h1, c1, R, rows);
    return AETHER_OK;
}
// The 1 .. 4 layers of prior_fc_out / encoder_fc_out on x [rows][in_size] through Y1 / Y2 [rows][hidden] into out [rows][out_size]
int nri_head_linear(const float* const* w, const float* const* b, int layers, int in_size, int hidden, int out_size, int64_t rows,
                    const float* x, float* Y1, float* Y2, float* out, hipStream_t st) {
    const float* cur = x;
    int cur_k = in_size;
    for (int l = 0; l < layers; ++l) {
        const bool last = l + 1 == layers;
        float* dst = last ? out : l % 2 == 0 ? Y1 : Y2;
        const int M = last ? out_size : hidden;
        if (s2s_linear(last ? 0 : 4, w[l], cur_k, b[l], cur, dst, M, cur_k, rows, M, nullptr, 0, 0, st)) return AETHER_EINVAL;
        cur = dst;
        cur_k = M;
    }
    return AETHER_OK;
}

// ---- 3b. the tail of the variable-N sequence encoders (Encoder.forward, aether_dynamicvars.py:588-670, dnri_dynamicvars.py:
// 463-542) on the mlp4 rows x [rows][h] of ALL frames: the LSTM step from the zero state (k_dyn_lstm_zero: the reference
// never writes the forward state back, and never runs reverse_rnn), then prior_fc_out(h1) and encoder_fc_out([h1 | 0]) layer
// by layer, the two heads' layers of the same depth in one launch.  The posterior head's first Linear reads the first R of its
// 2R input columns: its weight goes in with a row stride of 2R, no zero-padded copy of h1 is made.
struct NriSeqTail {
    const float* const* post_w; const float* const* post_b;      // encoder_fc_out, 1 .. 4 layers
    int post_layers, post_hidden;
    float *P1, *P2, *posterior_logits;                           // [rows][post_hidden] x 2 (unused with one layer), [rows][K]
    const int* status;                                           // k_dyn_lstm_zero's poison word, or null
};
int nri_seq_tail(const float* w_ih, const float* b_ih, const float* b_hh, const float* const* prior_w, const float* const* prior_b,
                 int prior_layers, int ph, const NriSeqTail& q, int h, int R, int K, int64_t rows, const float* x, float* h1,
                 float* Y1, float* Y2, float* prior_logits, hipStream_t st) {
    k_dyn_lstm_zero<<<dim3((unsigned)((rows + 63) / 64), (unsigned)(R / 16)), dim3(256), 0, st>>>(x, w_ih, b_ih, b_hh, h, R, rows,
                                                                                               q.status, h1);
    const float *pc = h1, *qc = h1;
    int pk = R, qk = R;
    for (int l = 0; l < std::max(prior_layers, q.post_layers); ++l) {
        S2SJobs T;
        T.n = 0;
        if (l < prior_layers) {
            const bool last = l + 1 == prior_layers;
            float* dst = last ? prior_logits : l % 2 == 0 ? Y1 : Y2;
            const int M = last ? K : ph;
            T.j[T.n++] = s2s_job(last ? 0 : 4, prior_w[l], pk, prior_b[l], pc, pk, dst, M, M, pk, rows);
            pc = dst; pk = M;
        }
        if (l < q.post_layers) {
            const bool last = l + 1 == q.post_layers;
            float* dst = last ? q.posterior_logits : l % 2 == 0 ? q.P1 : q.P2;
            const int M = last ? K : q.post_hidden;
            T.j[T.n++] = s2s_job(last ? 0 : 4, q.post_w[l], l == 0 ? 2 * R : qk, q.post_b[l], qc, qk, dst, M, M, qk, rows);
            qc = dst; qk = M;
        }
        if (int rc = s2s_launch_jobs(T, st)) return rc;
    }
    return AETHER_OK;
}

// ---- 4. the dNRI prior from mlp1's second layer (on X1a [Nn][h], the caller's node kernel's) to mlp4 -> out [E][h].
// first_jobs(T) adds what rides in the first launch (and flushes T itself where it fills up).  Receiver reduction between mlp2
// and mlp3: mean_div > 0 the in-edge sum / mean_div (k_s2s_segment_mean), 0 the plain sum (k_dyn_dnri_recv_sum)
struct NriDnriPrior {
    const float *bn_scale[4], *bn_shift[4];
    const void *img_w3[4], *img_m2s, *img_m2r, *img_m3_0, *img_ps, *img_pr, *img_m4e;
    const int64_t *send, *recv, *order, *rowptr;
    float mean_div;
    float *X1a, *X1, *Ps, *Pr, *T2, *X2, *X2n, *X3a, *X3, *T4, *out;
    int h; int64_t Nn, E;
};
extern "C++" template <class PriorParams, class FirstJobs>
int nri_dnri_prior(const PriorParams* p, const NriDnriPrior& c, FirstJobs&& first_jobs, hipStream_t st) {
    const int h = c.h;
    const int64_t Nn = c.Nn, E = c.E;
    S2SJobs T;
    T.n = 0;
    T.j[T.n++] = nri_with(s2s_job(4, p->mlp_w3[0], h, p->mlp_b3[0], c.X1a, h, c.X1, h, h, h, Nn), c.img_w3[0], c.bn_scale[0], c.bn_shift[0]);
    if (int rc = first_jobs(T)) return rc;
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    // node2edge, mlp2: the first Linear on [x_send | x_recv] as the node products of its two halves, no [E][2h] rows
    T.n = 0;
    T.j[T.n++] = nri_with(s2s_job(0, p->mlp_w0[1], 2 * h, p->mlp_b0[1], c.X1, h, c.Ps, h, h, h, Nn), c.img_m2s);
    T.j[T.n++] = nri_with(s2s_job(0, p->mlp_w0[1] + h, 2 * h, nullptr, c.X1, h, c.Pr, h, h, h, Nn), c.img_m2r);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    k_s2s_dnri_pair_elu<<<nri_blocks(E * (h / 4)), dim3(256), 0, st>>>(c.Ps, c.Pr, c.send, c.recv, c.T2, h, E);
    if (int rc = nri_one(st, s2s_job(4, p->mlp_w3[1], h, p->mlp_b3[1], c.T2, h, c.X2, h, h, h, E), c.img_w3[1], c.bn_scale[1],
                         c.bn_shift[1])) return rc;
    // edge2node over the receiver, mlp3
    if (c.mean_div > 0.0f)
        k_s2s_segment_mean<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(c.X2, c.order, c.rowptr, c.X2n, h, c.mean_div, nullptr);
    else
        k_dyn_dnri_recv_sum<<<dim3((unsigned)Nn), dim3(128), 0, st>>>(c.X2, c.order, c.rowptr, c.X2n, h);
    if (int rc = nri_one(st, s2s_job(4, p->mlp_w0[2], h, p->mlp_b0[2], c.X2n, h, c.X3a, h, h, h, Nn), c.img_m3_0)) return rc;
    if (int rc = nri_one(st, s2s_job(4, p->mlp_w3[2], h, p->mlp_b3[2], c.X3a, h, c.X3, h, h, h, Nn), c.img_w3[2], c.bn_scale[2],
                         c.bn_shift[2])) return rc;
    return nri_edge_mlp4(NriMlp4{p->mlp_w0[3], p->mlp_b0[3], p->mlp_w3[3], p->mlp_b3[3], c.bn_scale[3], c.bn_shift[3], c.img_ps,
                                 c.img_pr, c.img_m4e, c.img_w3[3], c.X3, c.X2, c.send, c.recv, c.Ps, c.Pr, c.T4, c.out, h, Nn, E}, st);
}

// ---- 5. the recurrent dNRI decoder from msg_fc1 to out_fc2.  sample [E][K] (hard) with its per-type lists / counts, scale
// [E][K]: what a message of type k is multiplied by.  node_products: false where A / S were made in the prior's launch.
// aggregate(): the caller's kernel from M [E][hd] to agg [Nn][hd].  -> dh_out, o2 [Nn][hd]; the output kernel is the caller's
struct NriDnriDecoder {
    const void *img_a[4], *img_s[4], *img_msg2[4], *img_hr, *img_hi, *img_hh, *img_out1, *img_out2;
    const float *x_in, *dh_in, *sample, *scale;
    const int64_t *lists, *send, *recv;
    const int* counts;
    float *A, *S, *Tm, *M, *agg, *hr, *hi, *hh, *o1, *o2, *dh_out;
    int ldx, hd, K, k0; int64_t Nn, E;
    bool node_products;
};
// The receiver | sender halves of msg_fc1[k] on the hidden state, as two jobs added to T
extern "C++" template <class DecoderParams>
void nri_dnri_msg1_pair(const DecoderParams* q, const NriDnriDecoder& d, int k, S2SJobs& T) {
    const int hd = d.hd;
    const size_t rows = (size_t)k * d.Nn * hd;
    T.j[T.n++] = nri_with(s2s_job(0, q->msg_fc1_w[k], 2 * hd, q->msg_fc1_b[k], d.dh_in, hd, d.A + rows, hd, hd, hd, d.Nn), d.img_a[k]);
    T.j[T.n++] = nri_with(s2s_job(0, q->msg_fc1_w[k] + hd, 2 * hd, nullptr, d.dh_in, hd, d.S + rows, hd, hd, hd, d.Nn), d.img_s[k]);
}
// msg_fc2 of every used type in one launch: rows through the type's list, times the sample's weight (act 3 / 2: with / without tanh)
int nri_dnri_msg2(int act, const float* const* w, const float* const* b, const NriDnriDecoder& d, hipStream_t st) {
    const int hd = d.hd;
    S2SJobs T;
    T.n = 0;
    for (int k = d.k0; k < d.K; ++k) {
        S2SJob J = s2s_job(act, w[k], hd, b[k], d.Tm + (size_t)k * d.E * hd, hd, d.M, hd, hd, hd, d.E);
        J.xidx = d.lists + (size_t)k * d.E; J.yidx = d.lists + (size_t)k * d.E; J.n_dev = d.counts + k;
        J.scale = d.scale + k; J.sstride = d.K; J.Wimg = d.img_msg2[k];
        T.j[T.n++] = J;
    }
    return s2s_launch_jobs(T, st);
}
extern "C++" template <class DecoderParams, class Aggregate>
int nri_dnri_decoder(const DecoderParams* q, const NriDnriDecoder& d, Aggregate&& aggregate, hipStream_t st) {
    const int hd = d.hd;
    const int64_t Nn = d.Nn, E = d.E;
    S2SJobs T;
    T.n = 0;
    for (int k = d.k0; d.node_products && k < d.K; ++k) nri_dnri_msg1_pair(q, d, k, T);
    if (int rc = s2s_launch_jobs(T, st)) return rc;                   // (no job: no launch)
    // first message layer of the sampled type, per edge, from its node products (rows of unsampled edges of M cleared)
    k_s2s_dnri_pair<false><<<nri_blocks(E * (hd / 4)), dim3(256), 0, st>>>(d.A, d.S, Nn, d.send, d.recv, d.sample, d.K, d.k0, d.Tm,
                                                                           d.M, hd, E);
    if (int rc = nri_dnri_msg2(3, q->msg_fc2_w, q->msg_fc2_b, d, st)) return rc;
    aggregate();
    // GRU-style gate on the raw inputs (ldx <= 6 columns), or on [inputs | field] of DNRIAether at D = 3 (9 columns)
    T.n = 0;
    T.j[T.n++] = nri_with(s2s_job(0, q->hidden_r_w, hd, nullptr, d.agg, hd, d.hr, hd, hd, hd, Nn), d.img_hr);
    T.j[T.n++] = nri_with(s2s_job(0, q->hidden_i_w, hd, nullptr, d.agg, hd, d.hi, hd, hd, hd, Nn), d.img_hi);
    T.j[T.n++] = nri_with(s2s_job(0, q->hidden_h_w, hd, nullptr, d.agg, hd, d.hh, hd, hd, hd, Nn), d.img_hh);
    if (int rc = s2s_launch_jobs(T, st)) return rc;
    if (d.ldx > 6)
        k_s2s_dnria_gate<<<nri_blocks(Nn * (hd / 4)), dim3(256), 0, st>>>(d.x_in, d.ldx, q->input_r_w, q->input_r_b, q->input_i_w,
                                                                          q->input_i_b, q->input_n_w, q->input_n_b, d.hr, d.hi, d.hh,
                                                                          d.dh_in, d.dh_out, hd, Nn);
    else
        k_s2s_dnri_gate<<<nri_blocks(Nn * (hd / 4)), dim3(256), 0, st>>>(d.x_in, d.ldx, q->input_r_w, q->input_r_b, q->input_i_w,
                                                                         q->input_i_b, q->input_n_w, q->input_n_b, d.hr, d.hi, d.hh,
                                                                         d.dh_in, d.dh_out, hd, Nn);
    if (int rc = nri_one(st, s2s_job(2, q->out1_w, hd, q->out1_b, d.dh_out, hd, d.o1, hd, hd, hd, Nn), d.img_out1)) return rc;
    return nri_one(st, s2s_job(2, q->out2_w, hd, q->out2_b, d.o1, hd, d.o2, hd, hd, hd, Nn), d.img_out2);
}

// ---- 6. the rollout loop of the seq2seq engine.  The state a step reads and the one it writes: x [Nn][2D], dh [Nn][hd]
// (null: the decoder has no state), h / c [E][R]; where the ping-pong state lies in the workspace (bytes), and its rows' sizes
struct S2SStateIn { const float *x, *dh, *h, *c; };
struct S2SStateOut { float *x, *dh, *h, *c; };
struct NriRolloutWs { size_t xa, da, db, ha, hb, ca, cb; int D, hd, R, K; int64_t Nn, E; };
// burn_in [T0][Nn][2D] teacher-forced, then `steps` steps from inputs; decoder_state (null: the decoder has none), h, c are
// read first and written last.  step(t, teacher, cur, uniform_t, next, edges_out_t, decode) -> status
extern "C++" template <class Step>
int nri_rollout(char* ws, const NriRolloutWs& o, int burn_in_steps, const float* burn_in, int steps, const float* inputs,
                float* decoder_state, float* h, float* c, const float* uniform, float* predictions, float* edges_out, Step&& step,
                hipStream_t st) {
    auto wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const size_t dbytes = (size_t)o.Nn * o.hd * 4, rbytes = (size_t)o.E * o.R * 4;
    const size_t ustep = (size_t)o.E * o.K, xstep = (size_t)o.Nn * 2 * o.D;
    // state ping-pong inside the workspace (the decoder's only when it has a state)
    float *dcur = decoder_state ? wp(o.da) : nullptr, *dnext = decoder_state ? wp(o.db) : nullptr;
    float *hcur = wp(o.ha), *hnext = wp(o.hb), *ccur = wp(o.ca), *cnext = wp(o.cb);
    if (dcur) HIP_OK(hipMemcpyAsync(dcur, decoder_state, dbytes, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(hcur, h, rbytes, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(ccur, c, rbytes, hipMemcpyDeviceToDevice, st));
    const float* xcur = burn_in_steps > 0 ? burn_in : inputs;
    for (int t = 0; t < burn_in_steps + steps; ++t) {
        // A burn-in step's prediction is discarded.  A decoder with a state still needs the step for it: the whole step, its
        // output into xa.  A stateless decoder (Markov, MLP): the prior only -- no sample, no decoder, no output.
        const bool teacher = t < burn_in_steps, decode = !teacher || decoder_state != nullptr;
        float* xout = !teacher ? predictions + (size_t)(t - burn_in_steps) * xstep : decode ? wp(o.xa) : nullptr;
        float* eout = (!teacher && edges_out) ? edges_out + (size_t)(t - burn_in_steps) * ustep : nullptr;
        if (int rc = step(t, teacher, S2SStateIn{xcur, dcur, hcur, ccur}, uniform + (size_t)t * ustep,
                          S2SStateOut{xout, dnext, hnext, cnext}, eout, decode)) return rc;
        std::swap(dcur, dnext); std::swap(hcur, hnext); std::swap(ccur, cnext);
        if (t + 1 < burn_in_steps) xcur = burn_in + (size_t)(t + 1) * xstep;
        else if (t + 1 == burn_in_steps) xcur = inputs;
        else xcur = xout;
    }
    if (dcur) HIP_OK(hipMemcpyAsync(decoder_state, dcur, dbytes, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(h, hcur, rbytes, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(c, ccur, rbytes, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipGetLastError());
    return AETHER_OK;
}
}  // namespace
