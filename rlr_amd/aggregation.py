"""Aggregation server (reference src/aggregation.py).

The server consumes a stacked (S, n_params) fp64 update matrix in sampled
order — on multi-GPU runs this is the RCCL all-gather result, identical on
every rank, and every rank applies the aggregate redundantly (deterministic,
zero extra traffic; SURVEY.md §2c call-site 3).  The dict-based reference
API (aggregation.py:19) is accepted too.

Rules (each a HIP kernel on the GPU path, ops/csrc/aggregation.hip):
  * RLR sign-vote (aggregation.py:48-54): sm = |sum_k sign(U_k)| per coord;
    lr = +server_lr where sm >= theta else -server_lr.  (The reference's
    in-place two-pass masking is only correct because -server_lr < theta
    for positive server_lr; this implementation is the explicit select and
    asserts that precondition — SURVEY.md §7 quirks.)
  * FedAvg (aggregation.py:57-64): sum_k n_k U_k / sum_k n_k, fp64, summed
    in sampled order for world-size-invariant bitwise results.
  * coordinate median (aggregation.py:66-69): torch.median column semantics
    (lower of the two middle values for even K).  K <= 64 runs the
    count-and-pick kernel; larger K sorts each column in LDS
    (ops/csrc/orderstat.hip) and selects the same element.
  * coordinate-wise trimmed mean (build addition, --aggr trmean; Yin et
    al., 2018): unweighted like the median; per coordinate drop
    b = floor(trim_frac * K) values from each end of the sorted column and
    average the rest, summed sequentially in ascending order in fp64 —
    agent-order invariant and bitwise equal between CPU and GPU.
    Without noise, trmean (and comed above K = 64) take ONE fused kernel:
    LDS sort + sign vote from the resident tile + fp32 apply.
  * Krum / Multi-Krum (build addition, --aggr krum; Blanchard et al.,
    2017): the one agent-wise rule.  D[i][j] = ||U_i - U_j||^2 (K x K fp64,
    exactly symmetric, zero diagonal, clamped at 0; on the GPU the fp64
    MFMA Gram kernel ops/csrc/pairdist.hip, on the CPU direct differences).
    With f = --krum_f agents assumed Byzantine and c = K - f - 2, score[i]
    sorts row i of D ascending, skips element 0 (the diagonal zero) and
    adds elements 1..c sequentially in ASCENDING order, times 1/c — exactly
    agg_orderstat(D, 1, c + 1) on the symmetric D.  The m = --krum_m agents
    with the lowest score are kept (stable sort: ties go to the lower
    sampled position; m = 0 means K - f, Multi-Krum; m = 1 is classic
    Krum) and averaged UNWEIGHTED like comed/trmean, accumulated in sampled
    order as acc += s_k * U_k with s_k in {1.0, 0.0}, times 1/m — the fused
    avg kernel with 0/1 weights is the same computation.  The RLR vote is
    taken over ALL K sampled updates: Krum decides what is averaged, the
    vote decides the direction.  Noise behaves as for avg on each backend.
    BatchNorm buffers are averaged unweighted over the same selection.
    Non-finite updates are out of scope (0 * inf is NaN).
  * geometric median / RFA (build addition, --aggr geomed; Pillutla et
    al., "Robust Aggregation for Federated Learning"): smoothed Weiszfeld,
    UNWEIGHTED like comed/trmean/krum, started at the plain mean.  With
    R = --geomed_iters and nu = --geomed_nu:
        a = ones(K)
        repeat R times:
            s     = a[0] + a[1] + ... + a[K-1]        sequential
            z_j   = (sum_k a[k] U[k][j]) * (1 / s)    sequential in k from 0
            d2[k] = sum_j (U[k][j] - z_j)^2           fp64
            a[k]  = 1 / max(nu, sqrt(d2[k]))
        aggregate = (sum_k a[k] U[k]) * (1 / sum a)
    i.e. the weighted-avg path with w = a; R = 0 is the unweighted mean.
    On the GPU the distances come from ops/csrc/geomed.hip (one streaming
    pass over U per iteration, no host sync inside the loop) and the last
    line is the fused avg kernel.  A smooth re-weighting, not a selection:
    the RLR vote is over ALL K, noise behaves as for avg on each backend,
    BatchNorm buffers are averaged with the same final weights.  The two
    backends agree to rounding, not bit for bit (the sum over n is chunked
    on the GPU); each is a pure function of its input.  last_weights holds
    the final a normalised to sum 1.
  * Bulyan (build addition, --aggr bulyan; El Mhamdi et al., "The Hidden
    Vulnerability of Distributed Learning in Byzantium", 2018): the
    agent-wise rule and the coordinate-wise rule composed.  With
    f = --bulyan_f agents assumed Byzantine and K >= 4f + 3 sampled
    (ValueError otherwise, checked per round):
      stage 1, selection: theta = K - 2f - 2 agents by ITERATED Krum over
        the one D = pairwise_sqdist(U).  All agents start alive; for
        t = 0 .. theta-1 let r = K - t and c = r - f - 2; score[i] of an
        alive agent sorts its distances to the other alive agents
        ascending, adds the first c sequentially in ascending order and
        multiplies by 1/c; the alive agent with the lowest score is selected
        and removed, ties to the lowest sampled position (stable sort).
        last_selected holds the theta positions ascending.  (The paper
        writes theta = K - 2f, which runs Krum on as few as 2f + 1 agents,
        below Krum's own 2f + 3; theta = K - 2f - 2 is what the authors'
        implementation uses and keeps r >= 2f + 3, c >= f + 1 in every
        iteration.)
      stage 2, per coordinate: sort the theta selected values ascending
        into s; m = (theta-1)//2, med = s[m] (the lower median, as comed
        takes it); beta = theta - 2f = K - 4f - 2 >= 1; grow a window from
        l = r = m, beta - 1 times:
            dl = med - s[l-1]   (+inf when l == 0)
            dr = s[r+1] - med   (+inf when r == theta-1)
            dl <= dr ? l -= 1 : r += 1              TIES GO LEFT
        agg = (s[l] + s[l+1] + ... + s[r]) * (1/beta), added sequentially
        in ascending order in fp64.
    Only subtractions, comparisons, ordered adds and one multiply: CPU and
    GPU agree bit for bit given the same selection, and the result does not
    depend on the agent order.  f = 0 selects K - 2 agents and averages all
    of them.  On the GPU the selection loop runs on device tensors without
    a host sync (a working copy of D whose dead rows and columns are +inf,
    scores from the order-statistic kernel, exactly krum's) and stage 2 is
    bulyan_k in ops/csrc/orderstat.hip: without noise ONE fused kernel
    sorts the selected rows in LDS, takes the vote over ALL K rows and
    applies.  Noise behaves as for trmean (the composed path only);
    --server_clip runs in front unchanged; BatchNorm buffers take the
    unweighted mean over the theta selected agents.  Non-finite updates are
    out of scope.
  * FoolsGold (build addition, --aggr foolsgold; Fung, Yoon, Beschastnikh,
    "The Limitations of Federated Learning in Sybil Settings", RAID 2020):
    the one rule with server state across rounds.  H (num_agents, n) fp64
    on the updates' device, zeros before the first round, holds every
    agent's summed updates; kappa = --foolsgold_kappa > 0; ids[0..K) the
    sampled agents, distinct.  Per round:
        0. H[ids[k]] += C[k]  for every k          one fp64 add per element
        1. G[i][j] = sum_t H[ids[i]][t] * H[ids[j]][t]   exactly symmetric
        2. den = sqrt(G[i][i] * G[j][j])
           cs[i][j] = den > 0 ? G[i][j] / den : 0  for i != j; cs[i][i] = 0
        3. v[i] = max_j cs[i][j]          the zero diagonal takes part
        4. for i != j: if v[i] < v[j]: cs[i][j] = (cs[i][j] * v[i]) / v[j]
           (pardoning; v is NOT recomputed)
        5. wv[i] = clamp(1 - max_j cs[i][j], 0, 1)   diagonal 0 again
        6. m = max_i wv[i]; if m > 0: wv[i] = wv[i] / m
           if wv[i] == 1.0: wv[i] = 0.99
        7. alpha[i] = clamp(kappa * (ln(wv[i] / (1 - wv[i])) + 0.5), 0, 1)
           (wv = 0 gives -inf, which clamps to 0)
        8. aggregate = (sum_k alpha[k] * C[k]) * (1.0 / K), sequential in
           sampled order from 0
    Steps 2-7 are foolsgold_weights() below, THE CPU rule.  The divisor is
    K, not sum(alpha): the rule scales each agent's learning rate, so with
    no sybils it is the unweighted mean and a round of all-sybil agents
    moves nothing (m == 0 leaves wv, alpha and the model where they are).
    Unweighted by data size like every other build addition.  On the GPU
    (K <= 512) step 0 is rows_add_k and steps 2-7 three small launches
    (ops/csrc/foolsgold.hip), step 1 the fp64 MFMA Gram stages of
    pairdist.hip over the sampled rows of H, step 8 the fused avg kernel
    with w = alpha and divisor K; no host sync.  The RLR vote is over ALL
    K, noise behaves as for avg on each backend, --server_clip runs in
    front so H accumulates the clipped rows, BatchNorm buffer deltas take
    (sum_k alpha[k] delta[k]) * (1 / K).  H is a pure function of the
    updates and bitwise equal between backends; G, and so alpha, agree to
    rounding (bounds in PARITY.md).  last_weights holds the raw alpha, not
    normalised (its sum may be 0); state_dict() carries H into the
    checkpoint.  Non-finite updates are out of scope.
  * sign (aggregation.py:71-75): sign(sum_k sign(U_k)).
  * server-side norm clipping (build addition, --server_clip > 0; Sun et
    al., "Can You Really Backdoor Federated Learning?", and the clipping
    half of DP-FedAvg): a stage IN FRONT of every rule above.
        norm[k] = sqrt(sum_j U[k][j]^2)               fp64
        tau     = server_clip                         --server_clip_mode fixed
        tau     = server_clip * lower median of norm  median: the
                  ((K-1)/2)-th smallest, as comed takes it
        s[k]    = norm[k] > tau ? tau / norm[k] : 1.0
        C[k][j] = s[k] * U[k][j]                      one rounding each
    Every rule sees C: avg, comed, sign, trmean, krum's distances and
    selection, geomed's weights, and the RLR vote (unchanged: s > 0 keeps
    every sign).  A zero row and a row with norm == tau keep s = 1 and
    their bits.  On the GPU ops/csrc/rowclip.hip (any K, three launches, no
    host sync) scales the matrix in place; CPU and force_eager build C in
    plain torch.  The backends agree to rounding (the sum over n is chunked
    on the GPU; bounds in PARITY.md).  BatchNorm buffer deltas are
    multiplied by the same s[k] before their mean.  last_clip_scale,
    last_clip_bound and last_norms hold s, tau and norm.  The older
    clip_updates below stays the disconnected reference-parity stub.
  * optional N(0, noise*clip) gaussian noise (aggregation.py:34-35) from a
    per-round derived stream; N(0, noise*server_clip) under a fixed
    --server_clip, whose bound is then the sensitivity (median mode keeps
    noise*clip: its bound is data-dependent and lives on the device).  The
    fused GPU avg path draws from the on-device philox stream, every other
    path from a torch CPU generator: a different, equally deterministic
    realization per backend (PARITY.md).
  * fused apply (aggregation.py:38-40): theta <- float32(theta + lr * agg).
"""

import torch
from torch.nn import functional as F

from .ops import ext, force_eager
from .options import check_foolsgold, check_geomed, check_server_clip
from .utils.rng import derive_seed, torch_gen


def _gpu(t):
    return t.is_cuda and not force_eager()


def _row_sum(rows, w=None):
    """sum_k w[k] * rows[k] (w omitted: sum_k rows[k]) — THE sequential sum
    of the CPU rules, which PARITY.md's bit-for-bit statements rest on:
    from zeros, added in place, in ascending k."""
    out = torch.zeros(rows.shape[1], dtype=torch.float64, device=rows.device)
    for k in range(rows.shape[0]):
        out += rows[k] if w is None else w[k] * rows[k]
    return out


def bulyan_window_mean(rows, beta):
    """Stage 2 of Bulyan in plain torch — THE CPU rule (module docstring):
    per column of rows (theta, n) the mean of the beta sorted values
    nearest the lower median, the window grown one step at a time with ties
    going left, summed in ascending order."""
    theta, n = rows.shape
    if not 1 <= beta <= theta:
        raise ValueError(f"beta={beta} must be in [1, theta] = [1, {theta}]")
    s = torch.sort(rows, dim=0).values
    col = torch.arange(n, device=rows.device)
    m = (theta - 1) // 2
    med = s[m]
    inf = torch.full_like(med, float('inf'))
    l = torch.full((n,), m, dtype=torch.long, device=rows.device)
    r = l.clone()
    for _ in range(beta - 1):
        dl = torch.where(l > 0, med - s[(l - 1).clamp(min=0), col], inf)
        dr = torch.where(r < theta - 1,
                         s[(r + 1).clamp(max=theta - 1), col] - med, inf)
        # beta <= theta keeps one side open; the edge tests keep l and r in
        # range for non-finite input too
        left = (r == theta - 1) | ((l > 0) & (dl <= dr))
        l = l - left.long()
        r = r + (~left).long()
    out = torch.zeros(n, dtype=rows.dtype, device=rows.device)
    for i in range(beta):
        out += s[l + i, col]
    return out * (1.0 / beta)


def foolsgold_weights(G, kappa):
    """Steps 2-7 of FoolsGold in plain torch — THE CPU rule (module
    docstring) and the reference for the kernel: (alpha, cs) from the Gram
    matrix G (K, K) of the sampled history rows, cs the cosine matrix of
    step 2, before pardoning.  No host sync."""
    g = G.diagonal()
    den = torch.sqrt(g.unsqueeze(1) * g.unsqueeze(0))
    zero = torch.zeros_like(G)
    cs = torch.where(den > 0, G / den, zero)
    cs.fill_diagonal_(0.0)
    v = cs.max(dim=1).values
    vi, vj = v.unsqueeze(1), v.unsqueeze(0)
    # never on the diagonal: v[i] < v[i] is false
    pardoned = torch.where(vi < vj, (cs * vi) / vj, cs)
    wv = (1.0 - pardoned.max(dim=1).values).clamp(0.0, 1.0)
    m = wv.max()
    wv = torch.where(m > 0, wv / m, wv)
    wv = torch.where(wv == 1.0, torch.full_like(wv, 0.99), wv)
    alpha = (kappa * (torch.log(wv / (1.0 - wv)) + 0.5)).clamp(0.0, 1.0)
    return alpha, cs


class Aggregation:
    def __init__(self, agent_data_sizes, n_params, poisoned_val_loader,
                 args, writer=None):
        self.agent_data_sizes = agent_data_sizes
        self.args = args
        self.writer = writer
        self.server_lr = args.server_lr
        self.n_params = n_params
        self.poisoned_val_loader = poisoned_val_loader
        self.cum_net_mov = 0.0
        # krum, bulyan: sampled positions kept last round
        self.last_selected = None
        # geomed: final weights, normalised; foolsgold: the raw alpha
        self.last_weights = None
        # foolsgold: (num_agents, n) fp64 summed updates per agent, on the
        # updates' device; None until the first round
        self.foolsgold_history = None
        # server_clip: last round's factors s (K), bound tau (0-d) and
        # pre-clip norms (K), on the updates' device
        self.last_clip_scale = None
        self.last_clip_bound = None
        self.last_norms = None

    # ------------------------------------------------------------- entry

    def aggregate_updates(self, global_model, agent_updates, cur_round,
                          agent_ids=None):
        """agent_updates: dict {agent_id: fp64 vec} (reference API) or a
        stacked (S, n) fp64 tensor with agent_ids giving the sampled order.
        With --server_clip a stacked matrix on the GPU is clipped IN PLACE;
        the dict form is stacked into a copy first, so the caller's tensors
        are untouched, as is a matrix on the CPU."""
        if isinstance(agent_updates, dict):
            agent_ids = list(agent_updates.keys())
            stacked = torch.stack([agent_updates[i] for i in agent_ids])
        else:
            stacked = agent_updates
            assert agent_ids is not None

        if self._server_clip() > 0:
            stacked = self.server_clip_updates(stacked)
            self._log_clip(agent_ids, cur_round)

        rule, w, span, subset, divisor = self._resolve(stacked, agent_ids,
                                                       cur_round)
        K = stacked.shape[0]
        rlr = self.args.robustLR_threshold > 0

        if _gpu(stacked) and w is not None:
            # headline path: ONE fused kernel does sign-vote + weighted avg
            # + noise + fp32 apply in a single pass over the K x n matrix
            # (vote over all K, whatever the weights)
            noise_std = self._noise_std() if self.args.noise > 0 else 0.0
            seed = derive_seed(self.args.seed, 'noise', cur_round)
            ext().fused_avg_rlr_apply(
                stacked, w, global_model.flat_params, rlr,
                float(self.args.robustLR_threshold), float(self.server_lr),
                float(noise_std), seed, 0, False,
                0.0 if divisor is None else float(divisor))
            return

        if (_gpu(stacked) and span is not None and self.args.noise == 0
                and K <= ext().orderstat_max_k()
                and (self.args.aggr == 'trmean' or K > 64)):
            # order-statistic rules: ONE fused kernel sorts each column in
            # LDS, takes the vote from the resident tile and applies.  The
            # median of K <= 64 stays composed: its count-and-pick kernel
            # is the faster one there (docs/KERNELS.md)
            ext().orderstat_rlr_apply(
                stacked, span[0], span[1], global_model.flat_params, rlr,
                float(self.args.robustLR_threshold), float(self.server_lr),
                False)
            return

        if (_gpu(stacked) and subset is not None and self.args.noise == 0
                and K <= ext().bulyan_max_k()):
            # bulyan: ONE fused kernel sorts the selected rows of each
            # column in LDS, trims around their median, takes the vote over
            # all K rows and applies
            sel, theta, beta = subset
            ext().bulyan_rlr_apply(
                stacked, self._bulyan_perm(sel, K), theta, beta,
                global_model.flat_params, rlr,
                float(self.args.robustLR_threshold), float(self.server_lr),
                False)
            return

        # composed path: vote, rule, noise, apply
        lr_vector = self.compute_robustLR(stacked) if rlr else None
        agg = rule(stacked)
        if self.args.noise > 0:
            agg = agg + self._noise(cur_round, agg.device, agg.dtype)
        self._apply(global_model, lr_vector, agg)

    def _resolve(self, stacked, agent_ids, cur_round):
        """What --aggr decides for this round, looked at in this one place:
        (rule, weights, span, subset, divisor).  weights: for a weighted
        mean of the rows, divided by divisor (None: by their sum); span:
        [lo, hi) of each sorted column to average; subset: (selected
        positions, theta, beta) for bulyan's trimmed mean around the median
        of the selected rows; none of them for sign.
        rule(stacked) is the aggregate as the composed path computes it.
        Sets last_selected / last_weights and logs what the rule chose."""
        aggr, K, dev = self.args.aggr, stacked.shape[0], stacked.device
        if aggr == 'avg':
            w = self._weights(agent_ids, dev)
            return ((lambda U: self._mean(U, w, self._avg_mean)), w, None,
                    None, None)
        if aggr == 'krum':
            self.last_selected = self.krum_select(stacked)
            self._log_krum(agent_ids, cur_round)
            w = self._krum_weights(K, dev)
            return ((lambda U: self._mean(U, w, self._krum_mean)), w, None,
                    None, None)
        if aggr == 'geomed':
            a = self.geomed_weights(stacked)
            self.last_weights = a / a.sum()
            self._log_geomed(agent_ids, cur_round)
            return ((lambda U: self._mean(U, a, self._geomed_mean)), a, None,
                    None, None)
        if aggr == 'foolsgold':
            alpha = self.last_weights = self.foolsgold_alpha(stacked,
                                                             agent_ids)
            self._log_foolsgold(agent_ids, cur_round)
            return ((lambda U: self._foolsgold_mean(U, alpha)), alpha, None,
                    None, K)
        if aggr == 'bulyan':
            theta, beta = self._bulyan_counts(K)
            sel = self.last_selected = self.bulyan_select(stacked)
            self._log_bulyan(agent_ids, cur_round)
            return ((lambda U: self._bulyan_trim(U, sel)), None, None,
                    (sel, theta, beta), None)
        if aggr == 'comed':
            return self.agg_comed, None, self._comed_span(K), None, None
        if aggr == 'trmean':
            return self.agg_trmean, None, self._trim_span(K), None, None
        if aggr == 'sign':
            return self.agg_sign, None, None, None, None
        raise ValueError(aggr)

    # ------------------------------------------------------- server clip

    def _server_clip(self):
        return float(getattr(self.args, 'server_clip', 0.0))

    def _server_clip_mode(self):
        return getattr(self.args, 'server_clip_mode', 'fixed')

    def server_clip_updates(self, stacked):
        """The clipped matrix C[k] = s[k] * U[k] (module docstring); on the
        GPU `stacked` itself, scaled in place.  Remembers s, tau and the
        pre-clip norms in last_clip_scale / last_clip_bound / last_norms."""
        value = self._server_clip()
        mode = self._server_clip_mode()
        check_server_clip(value, mode)
        if _gpu(stacked):
            s, norm, tau = ext().rowclip_(stacked, value, mode == 'median')
        else:
            K = stacked.shape[0]
            norm = torch.sqrt((stacked * stacked).sum(1))
            if mode == 'median':
                tau = value * torch.sort(norm).values[(K - 1) // 2]
            else:
                tau = torch.tensor(value, dtype=torch.float64,
                                   device=stacked.device)
            s = torch.where(norm > tau, tau / norm, torch.ones_like(norm))
            stacked = s.unsqueeze(1) * stacked
        self.last_clip_scale, self.last_clip_bound = s, tau
        self.last_norms = norm
        return stacked

    def _log_clip(self, agent_ids, cur_round):
        if self.writer:
            s = self.last_clip_scale.cpu()
            bad = [p for p, i in enumerate(agent_ids)
                   if i < self.args.num_corrupt]
            self.writer.add_scalar('Clip/Bound', float(self.last_clip_bound),
                                   cur_round)
            self.writer.add_scalar('Clip/Frac_Clipped',
                                   float((s < 1.0).double().mean()),
                                   cur_round)
            self.writer.add_scalar('Clip/Corrupt_Scale_Mean',
                                   float(s[bad].mean()) if bad else 1.0,
                                   cur_round)

    # ------------------------------------------------------------- rules

    def compute_robustLR(self, stacked: torch.Tensor) -> torch.Tensor:
        assert self.server_lr > 0 and self.args.robustLR_threshold > 0
        if _gpu(stacked):
            return ext().rlr_vote(stacked, float(self.args.robustLR_threshold),
                                  float(self.server_lr))
        sm = torch.abs(torch.sign(stacked).sum(dim=0))
        return torch.where(sm >= self.args.robustLR_threshold,
                           torch.full_like(sm, self.server_lr),
                           torch.full_like(sm, -self.server_lr))

    def _weights(self, agent_ids, device):
        w = torch.tensor([float(self.agent_data_sizes[i]) for i in agent_ids],
                         dtype=torch.float64, device=device)
        return w

    @staticmethod
    def _mean(stacked, w, cpu_mean):
        """Mean of the rows under the weights w: the agg_avg kernel, or in
        plain torch one of the three cpu_mean below.  They differ only in
        how they divide, in the last bit; PARITY.md pins each."""
        return (ext().agg_avg(stacked, w) if _gpu(stacked)
                else cpu_mean(stacked, w))

    @staticmethod
    def _avg_mean(stacked, w):
        # summed in sampled order (world-size invariant)
        return _row_sum(stacked, w) / w.sum()

    def agg_avg(self, stacked, agent_ids):
        return self._mean(stacked, self._weights(agent_ids, stacked.device),
                          self._avg_mean)

    @staticmethod
    def _comed_span(K):
        """The lower median, torch.median's: sorted element (K - 1) // 2."""
        return (K - 1) // 2, (K - 1) // 2 + 1

    def agg_comed(self, stacked):
        # the count-and-pick kernel re-reads the column K times per value
        # and is bound to K <= 64; above that the LDS sorting kernel selects
        # the same element (a median is a selection, so bitwise identical);
        # beyond its K limit fall back to torch.median (same semantics)
        K = stacked.shape[0]
        if _gpu(stacked):
            if K <= 64:
                return ext().agg_comed(stacked)
            if K <= ext().orderstat_max_k():
                return ext().agg_orderstat(stacked, *self._comed_span(K),
                                           False, 0.0, 0.0)[0]
        return torch.median(stacked, dim=0).values

    def _trim_count(self, K):
        """b = floor(trim_frac * K) values dropped from each end."""
        b = int(self.args.trim_frac * K)
        if K - 2 * b < 1:
            raise ValueError(
                f"trim_frac={self.args.trim_frac} trims {b} of K={K} sampled "
                f"agents from each end and leaves nothing to average")
        return b

    def _trim_span(self, K):
        b = self._trim_count(K)
        return b, K - b

    def agg_trmean(self, stacked):
        """Coordinate-wise trimmed mean (Yin et al., 2018), unweighted like
        comed: per coordinate sort the K values, drop b from each end and
        average the rest.  The kept values are summed sequentially in
        ASCENDING order in fp64 and multiplied by 1/(K-2b) — the HIP kernel
        does exactly this, so CPU and GPU agree bit for bit and the result
        does not depend on the agent order."""
        K = stacked.shape[0]
        lo, hi = self._trim_span(K)
        if _gpu(stacked) and K <= ext().orderstat_max_k():
            return ext().agg_orderstat(stacked, lo, hi, False, 0.0, 0.0)[0]
        kept = torch.sort(stacked, dim=0).values[lo:hi]
        return _row_sum(kept) * (1.0 / (hi - lo))

    # -------------------------------------------------------------- krum

    def _krum_counts(self, K):
        """(c, m): neighbours scored per agent and agents kept."""
        f, m = self.args.krum_f, self.args.krum_m
        if f < 0 or K - f - 2 < 1:
            raise ValueError(
                f"krum_f={f} leaves K - f - 2 = {K - f - 2} neighbours to "
                f"score each of K={K} sampled agents by; need at least 1")
        if m == 0:
            m = K - f
        if not 1 <= m <= K - f:
            raise ValueError(
                f"krum_m={m} must be in [1, K - krum_f] = [1, {K - f}] for "
                f"K={K} sampled agents")
        return K - f - 2, m

    def pairwise_sqdist(self, stacked):
        """D[i][j] = ||U_i - U_j||^2: exactly symmetric, zero diagonal,
        no entry below 0."""
        K = stacked.shape[0]
        if _gpu(stacked):
            if K <= ext().pairdist_max_k():
                return ext().pairwise_sqdist(stacked)
            # above the kernel's K limit: Gram form in torch, one triangle
            # mirrored so the properties hold whatever the BLAS does
            G = stacked @ stacked.T
            g = G.diagonal()
            D = (g.unsqueeze(1) + g.unsqueeze(0) - 2.0 * G).clamp_(min=0.0)
            D = torch.triu(D, diagonal=1)
            return D + D.T
        D = torch.empty(K, K, dtype=torch.float64, device=stacked.device)
        for i in range(K):
            D[i] = ((stacked - stacked[i]) ** 2).sum(1)
        D = torch.triu(D, diagonal=1)
        return D + D.T

    def krum_scores(self, D):
        """score[i] = mean of the c smallest distances from agent i to the
        others, summed in ascending order."""
        K = D.shape[0]
        c, _ = self._krum_counts(K)
        if _gpu(D) and K <= ext().orderstat_max_k():
            # D is symmetric: sorting its columns sorts its rows
            return ext().agg_orderstat(D.contiguous(), 1, c + 1, False,
                                       0.0, 0.0)[0]
        return _row_sum(torch.sort(D, dim=0).values[1:c + 1]) * (1.0 / c)

    def krum_select(self, stacked):
        """Sampled positions of the m lowest-score agents, ascending."""
        _, m = self._krum_counts(stacked.shape[0])
        scores = self.krum_scores(self.pairwise_sqdist(stacked))
        order = torch.sort(scores, stable=True).indices
        return torch.sort(order[:m]).values

    def _krum_weights(self, K, device):
        w = torch.zeros(K, dtype=torch.float64, device=device)
        w[self.last_selected.to(device)] = 1.0
        return w

    def _krum_mean(self, stacked, w):
        return _row_sum(stacked, w) * (1.0 / self.last_selected.numel())

    def agg_krum(self, stacked):
        """Unweighted mean of the Krum-selected updates (module docstring).
        Remembers the selection in last_selected."""
        self.last_selected = self.krum_select(stacked)
        w = self._krum_weights(stacked.shape[0], stacked.device)
        return self._mean(stacked, w, self._krum_mean)

    def _log_krum(self, agent_ids, cur_round):
        if self.writer:
            n_bad = sum(1 for p in self.last_selected.tolist()
                        if agent_ids[p] < self.args.num_corrupt)
            self.writer.add_scalar('Krum/Corrupt_Selected', n_bad, cur_round)

    # ------------------------------------------------------------ bulyan

    def _bulyan_counts(self, K):
        """(theta, beta): agents selected, values averaged per coordinate."""
        f = self.args.bulyan_f
        if f < 0 or K < 4 * f + 3:
            raise ValueError(
                f"bulyan_f={f} needs K >= 4 f + 3 = {4 * f + 3} sampled "
                f"agents, got K={K}")
        return K - 2 * f - 2, K - 4 * f - 2

    def bulyan_picks(self, D):
        """Stage 1 given the distances D (K, K): iterated Krum, the theta
        selected positions ascending.  One loop for both backends and no
        host sync in it: dead rows and columns of the working copy are
        +inf, so a dead agent scores +inf and an alive one, whose sorted
        column is its own 0, the alive others and then +inf, scores exactly
        the rule's sum.  The scores are krum_scores' on either backend."""
        K = D.shape[0]
        f = self.args.bulyan_f
        theta, _ = self._bulyan_counts(K)
        Dw = D.clone(memory_format=torch.contiguous_format)
        kernel = _gpu(D) and K <= ext().orderstat_max_k()
        picks = []
        for t in range(theta):
            c = K - t - f - 2
            if kernel:
                scores = ext().agg_orderstat(Dw, 1, c + 1, False, 0.0, 0.0)[0]
            else:
                scores = (_row_sum(torch.sort(Dw, dim=0).values[1:c + 1])
                          * (1.0 / c))
            win = torch.sort(scores, stable=True).indices[:1]
            Dw.index_fill_(0, win, float('inf'))
            Dw.index_fill_(1, win, float('inf'))
            picks.append(win)
        return torch.sort(torch.cat(picks)).values

    def bulyan_select(self, stacked):
        """Sampled positions of the theta agents iterated Krum selects,
        ascending."""
        self._bulyan_counts(stacked.shape[0])
        return self.bulyan_picks(self.pairwise_sqdist(stacked))

    @staticmethod
    def _bulyan_perm(sel, K):
        """The K row indices as int32, the selected ones first (both parts
        ascending), built on sel's device without a host sync."""
        rest = torch.ones(K, dtype=torch.int8, device=sel.device)
        rest[sel] = 0
        return torch.sort(rest, stable=True).indices.to(torch.int32)

    def _bulyan_trim(self, stacked, sel):
        """Stage 2 over the rows sel of stacked."""
        K = stacked.shape[0]
        theta, beta = self._bulyan_counts(K)
        if _gpu(stacked) and K <= ext().bulyan_max_k():
            return ext().bulyan_trim(stacked, self._bulyan_perm(sel, K),
                                     theta, beta, False, 0.0, 0.0)[0]
        # the CPU rule; above the kernel's K limit the same on the device
        return bulyan_window_mean(stacked[sel], beta)

    def agg_bulyan(self, stacked):
        """Bulyan aggregate of the updates (module docstring), fp64.
        Remembers the selection in last_selected."""
        self.last_selected = self.bulyan_select(stacked)
        return self._bulyan_trim(stacked, self.last_selected)

    def _log_bulyan(self, agent_ids, cur_round):
        if self.writer:
            n_bad = sum(1 for p in self.last_selected.tolist()
                        if agent_ids[p] < self.args.num_corrupt)
            self.writer.add_scalar('Bulyan/Corrupt_Selected', n_bad,
                                   cur_round)

    # ------------------------------------------------------------ geomed

    def _geomed_loop(self, stacked):
        """The rule as written in the module docstring, in plain torch."""
        K = stacked.shape[0]
        nu = float(self.args.geomed_nu)
        a = torch.ones(K, dtype=torch.float64, device=stacked.device)
        for _ in range(int(self.args.geomed_iters)):
            d2 = ((stacked - self._geomed_mean(stacked, a)) ** 2).sum(1)
            a = 1.0 / torch.sqrt(d2).clamp(min=nu)
        return a

    def geomed_weights(self, stacked):
        """Raw Weiszfeld weights a[k] = 1 / max(nu, ||U_k - z||) after
        geomed_iters updates from a = ones (ones for geomed_iters = 0)."""
        check_geomed(self.args.geomed_iters, self.args.geomed_nu)
        if _gpu(stacked) and stacked.shape[0] <= ext().geomed_max_k():
            return ext().geomed_weights(stacked, int(self.args.geomed_iters),
                                        float(self.args.geomed_nu))[0]
        # the CPU reference; above the kernel's K limit the same loop on
        # the device
        return self._geomed_loop(stacked)

    @staticmethod
    def _geomed_mean(stacked, a):
        """(sum_k a[k] U[k]) * (1 / sum a), both sums sequential from 0."""
        # a as a (K, 1) matrix: its row sum is a[0] + a[1] + ... in order
        return _row_sum(stacked, a) * (1.0 / _row_sum(a.unsqueeze(1)))

    def agg_geomed(self, stacked):
        """Smoothed-Weiszfeld geometric median of the updates (module
        docstring), fp64.  Remembers the normalised weights in
        last_weights."""
        a = self.geomed_weights(stacked)
        self.last_weights = a / a.sum()
        return self._mean(stacked, a, self._geomed_mean)

    def _log_geomed(self, agent_ids, cur_round):
        if self.writer:
            bad = [p for p, i in enumerate(agent_ids)
                   if i < self.args.num_corrupt]
            share = float(self.last_weights[bad].sum()) if bad else 0.0
            self.writer.add_scalar('Geomed/Corrupt_Weight', share, cur_round)

    # --------------------------------------------------------- foolsgold

    def _foolsgold_ids(self, agent_ids):
        """The sampled ids as a CPU int64 vector, checked: distinct and
        below num_agents."""
        ids = [int(i) for i in agent_ids]
        A = int(self.args.num_agents)
        if any(i < 0 or i >= A for i in ids):
            raise ValueError(
                f"foolsgold: agent ids must be in [0, num_agents) = "
                f"[0, {A}), got {ids}")
        if len(set(ids)) != len(ids):
            raise ValueError(
                f"foolsgold: agent ids must be distinct, got {ids}")
        return torch.tensor(ids, dtype=torch.long)

    @staticmethod
    def _foolsgold_kernel(t, K):
        return _gpu(t) and K <= ext().foolsgold_max_k()

    def foolsgold_accumulate(self, stacked, agent_ids):
        """Step 0: H[ids[k]] += stacked[k].  H is allocated, as zeros on
        stacked's device, by the first call."""
        idx = self._foolsgold_ids(agent_ids)
        K, n = stacked.shape
        if len(idx) != K:
            raise ValueError(
                f"foolsgold: {len(idx)} agent ids for {K} updates")
        H = self.foolsgold_history
        if H is None:
            H = self.foolsgold_history = torch.zeros(
                int(self.args.num_agents), n, dtype=torch.float64,
                device=stacked.device)
        if H.shape[1] != n or H.device != stacked.device:
            raise ValueError(
                f"foolsgold: the history is {tuple(H.shape)} on {H.device}, "
                f"the updates are {tuple(stacked.shape)} on {stacked.device}")
        if self._foolsgold_kernel(stacked, K):
            ext().rows_add_(H, idx, stacked.contiguous())
        else:
            H.index_add_(0, idx.to(H.device), stacked)

    def foolsgold_gram(self, agent_ids):
        """Step 1: the (K, K) Gram matrix of the sampled history rows,
        exactly symmetric."""
        idx = self._foolsgold_ids(agent_ids)
        H, K = self.foolsgold_history, len(idx)
        if self._foolsgold_kernel(H, K):
            return ext().gram_rows(H, idx)
        Hs = H[idx.to(H.device)]
        if _gpu(H):
            # above the kernel's K limit: one triangle mirrored, so G is
            # symmetric whatever the BLAS does
            G = Hs @ Hs.T
        else:
            G = torch.empty(K, K, dtype=torch.float64, device=H.device)
            for i in range(K):
                G[i] = (Hs * Hs[i]).sum(1)
        up = torch.triu(G, diagonal=1)
        return up + up.T + torch.diag(G.diagonal())

    def foolsgold_alpha(self, stacked, agent_ids):
        """Steps 0-7: adds this round to the history and returns the raw
        alpha (K) of the sampled agents.  One call is one round."""
        kappa = float(self.args.foolsgold_kappa)
        check_foolsgold(kappa)
        self.foolsgold_accumulate(stacked, agent_ids)
        G = self.foolsgold_gram(agent_ids)
        if self._foolsgold_kernel(G, G.shape[0]):
            return ext().foolsgold_weights(G, kappa)[0]
        # the CPU rule; above the kernel's K limit the same on the device
        return foolsgold_weights(G, kappa)[0]

    @staticmethod
    def _foolsgold_mean(stacked, alpha):
        """(sum_k alpha[k] U[k]) * (1 / K), the sum sequential from 0."""
        K = stacked.shape[0]
        if _gpu(stacked):
            return ext().agg_avg(stacked, alpha, float(K))
        return _row_sum(stacked, alpha) * (1.0 / K)

    def agg_foolsgold(self, stacked, agent_ids):
        """FoolsGold aggregate of the updates (module docstring), fp64; one
        call is one round of the history.  Remembers the raw alpha in
        last_weights."""
        self.last_weights = self.foolsgold_alpha(stacked, agent_ids)
        return self._foolsgold_mean(stacked, self.last_weights)

    def _log_foolsgold(self, agent_ids, cur_round):
        """The one place that syncs for logging."""
        if self.writer:
            a = self.last_weights.cpu()
            bad = [p for p, i in enumerate(agent_ids)
                   if i < self.args.num_corrupt]
            good = [p for p, i in enumerate(agent_ids)
                    if i >= self.args.num_corrupt]
            if bad:
                self.writer.add_scalar('FoolsGold/Corrupt_Alpha_Mean',
                                       float(a[bad].mean()), cur_round)
            if good:
                self.writer.add_scalar('FoolsGold/Honest_Alpha_Mean',
                                       float(a[good].mean()), cur_round)

    def state_dict(self):
        """The server state a checkpoint has to carry: the FoolsGold
        history once it exists, nothing for every other rule."""
        if (self.args.aggr == 'foolsgold'
                and self.foolsgold_history is not None):
            return {'foolsgold_history': self.foolsgold_history}
        return {}

    def load_state_dict(self, state, device=None):
        """Restores what state_dict() returned, onto `device` (default:
        where the saved tensor lives)."""
        H = state.get('foolsgold_history')
        if H is None:
            return
        want = (int(self.args.num_agents), self.n_params)
        if tuple(H.shape) != want or H.dtype != torch.float64:
            raise ValueError(
                f"foolsgold history is {tuple(H.shape)} {H.dtype}; this run "
                f"needs {want} torch.float64")
        self.foolsgold_history = H.to(device or H.device).clone()

    def agg_sign(self, stacked):
        if _gpu(stacked):
            return ext().agg_sign(stacked)
        return torch.sign(torch.sign(stacked).sum(dim=0))

    def _noise_std(self):
        """noise * server_clip when the server enforces a fixed bound (its
        bound is then the sensitivity: clip + noise is DP-FedAvg), noise *
        clip otherwise — also in median mode, whose bound lives on the
        device and changes with the data."""
        if self._server_clip() > 0 and self._server_clip_mode() == 'fixed':
            return self.args.noise * self._server_clip()
        return self.args.noise * self.args.clip

    def _noise(self, cur_round, device, dtype):
        g = torch_gen(self.args.seed, 'noise', cur_round)
        n = torch.normal(mean=0.0, std=self._noise_std(),
                         size=(self.n_params,), generator=g)
        return n.to(device=device, dtype=dtype)

    def _apply(self, global_model, lr_vector, agg):
        """theta <- float32(theta + lr * agg) (reference aggregation.py:38-40)."""
        p = global_model.flat_params
        if _gpu(p):
            ext().apply_update(p, agg,
                               lr_vector if lr_vector is not None
                               else torch.empty(0, device=p.device),
                               float(self.server_lr))
            return
        if lr_vector is None:
            new = p.double() + self.server_lr * agg
        else:
            new = p.double() + lr_vector.double() * agg
        p.copy_(new.float())

    def _buffer_weights(self, agent_ids, device):
        """What the rule last decided about the agents, read back from
        last_selected / last_weights; data sizes for the rules that decide
        nothing about them."""
        if self.args.aggr in ('krum', 'bulyan'):
            return self._krum_weights(len(agent_ids), device)
        if self.args.aggr in ('geomed', 'foolsgold'):
            return self.last_weights.to(device)
        return self._weights(agent_ids, device)

    def _buffer_divisor(self, K):
        """What the weighted mean of the buffers divides by: None for the
        sum of the weights, K under foolsgold, as for the parameters."""
        return K if self.args.aggr == 'foolsgold' else None

    def aggregate_buffers(self, global_model, buffer_deltas, agent_ids):
        """FedAvg-BN: data-weighted mean of BatchNorm running-stat deltas
        (build extension — the reference has no BN).  Under krum and bulyan:
        the unweighted mean over the agents selected for the parameters;
        under foolsgold (sum_k alpha[k] delta[k]) * (1 / K).  Under
        --server_clip agent k's delta is first multiplied by the s[k] its
        update was clipped with."""
        if global_model.n_buffers == 0 or buffer_deltas is None:
            return
        if isinstance(buffer_deltas, (list, tuple)) and not buffer_deltas:
            return
        dev = (buffer_deltas.device if isinstance(buffer_deltas, torch.Tensor)
               else buffer_deltas[0].device)
        w = self._buffer_weights(agent_ids, dev)
        if isinstance(buffer_deltas, list):
            buffer_deltas = torch.stack(buffer_deltas)
        if self._server_clip() > 0 and self.last_clip_scale is not None:
            # an agent's buffer delta shrinks with its update
            buffer_deltas = (buffer_deltas.double()
                             * self.last_clip_scale.to(dev).unsqueeze(1))
        div = self._buffer_divisor(buffer_deltas.shape[0])
        if _gpu(buffer_deltas):
            # same weighted-mean HIP kernel as the parameter path (the
            # buffer matrix is tiny — K x ~10k — so the fp64 round-trip
            # is free and keeps one aggregation code path)
            mean = ext().agg_avg(buffer_deltas.double().contiguous(), w,
                                 0.0 if div is None else float(div))
        elif div is None:
            mean = (buffer_deltas.double()
                    * (w / w.sum()).unsqueeze(1)).sum(dim=0)
        else:
            mean = ((buffer_deltas.double() * w.unsqueeze(1)).sum(dim=0)
                    * (1.0 / div))
        global_model.flat_buffers.add_(mean.to(global_model.flat_buffers.dtype))

    # ------------------------------------------------- server-side extras

    def clip_updates(self, agent_updates_dict):
        """Server-side L2 projection (reference aggregation.py:77-81;
        disconnected from the main path there and here — the client does it
        per batch, agent.py:54-60)."""
        for update in agent_updates_dict.values():
            l2 = torch.norm(update, p=2)
            update.div_(max(1, l2 / self.args.clip))

    def plot_norms(self, agent_updates_dict, cur_round, norm=2):
        """Honest vs corrupt update-norm scalars (reference
        aggregation.py:83-100)."""
        honest, corrupt = [], []
        for key, upd in agent_updates_dict.items():
            (corrupt if key < self.args.num_corrupt else honest).append(upd)
        if honest and self.writer:
            avg = sum(torch.norm(u, p=norm) for u in honest) / len(honest)
            self.writer.add_scalar(f'Norms/Avg_Honest_L{norm}', avg, cur_round)
        if corrupt and self.writer:
            avg = sum(torch.norm(u, p=norm) for u in corrupt) / len(corrupt)
            self.writer.add_scalar(f'Norms/Avg_Corrupt_L{norm}', avg, cur_round)

    # -------------------------------------------- Fisher diagnostics

    def comp_diag_fisher(self, model_params, poisoned_eval, adv=True):
        """Diagonal Fisher over the poisoned validation tensors — the
        per-parameter squared-gradient of the summed target logit
        (reference aggregation.py:102-129 semantics, tensor-resident and
        on-device; the reference's probe model never leaves the CPU,
        SURVEY.md §7 quirks).  adv=True scores against the TRUE labels,
        adv=False against the attacker's base class.  The reference
        gathers raw LOGITS (its log_softmax result is discarded,
        aggregation.py:123) — behavior kept."""
        from . import models as M
        from .flatmodel import FlatParamModel
        X, Y = poisoned_eval
        probe = FlatParamModel(
            M.get_model(self.args.data, getattr(self.args, 'model', None)),
            X.device)
        probe.load_vector(model_params.float())
        probe.eval()
        fisher = torch.zeros_like(probe.flat_params)
        n = X.shape[0]
        for lo in range(0, n, self.args.bs):
            xb = X[lo:lo + self.args.bs]
            yb = (Y[lo:lo + self.args.bs] if adv
                  else torch.full_like(Y[lo:lo + self.args.bs],
                                       self.args.base_class))
            probe.zero_grad()
            logits = probe(xb)
            F.log_softmax(logits, dim=1)  # parity: computed, unused
            logits.gather(1, yb.view(-1, 1)).sum().backward()
            fisher += probe.flat_grads.square() / n
        return fisher.detach()

    def plot_sign_agreement(self, robustLR, cur_global_params,
                            new_global_params, cur_round):
        """Sign-agreement diagnostics (reference aggregation.py:132-191
        scalar names/semantics): how much of this round's movement landed
        on coordinates the attacker's Fisher ranks as important but the
        honest Fisher does not — split by whether the RLR vote pushed the
        coordinate forward (+server_lr) or flipped it (-server_lr)."""
        update = new_global_params - cur_global_params
        n_par = update.numel()

        def top_mask(fisher):
            m = torch.zeros(n_par, dtype=torch.bool, device=update.device)
            m[fisher.topk(self.args.top_frac).indices] = True
            return m

        adv_top = top_mask(self.comp_diag_fisher(cur_global_params,
                                                 self.poisoned_val_loader))
        hon_top = top_mask(self.comp_diag_fisher(cur_global_params,
                                                 self.poisoned_val_loader,
                                                 adv=False))
        fwd = robustLR.view(-1) == self.server_lr    # vote kept direction
        flipped = robustLR.view(-1) == -self.server_lr

        def l2_on(mask):
            return update[mask].norm().item()

        scalars = {
            'Sign/Adv_Maxim_L2': l2_on(fwd & adv_top & ~hon_top),
            'Sign/Hon_Maxim_L2': l2_on(fwd & hon_top & ~adv_top),
            'Sign/Adv_Minim_L2': l2_on(flipped & adv_top & ~hon_top),
            'Sign/Hon_Minim_L2': l2_on(flipped & hon_top & ~adv_top),
        }
        scalars['Sign/Adv_Net_L2'] = (scalars['Sign/Adv_Maxim_L2']
                                      - scalars['Sign/Adv_Minim_L2'])
        scalars['Sign/Hon_Net_L2'] = (scalars['Sign/Hon_Maxim_L2']
                                      - scalars['Sign/Hon_Minim_L2'])
        self.cum_net_mov += (scalars['Sign/Hon_Net_L2']
                             - scalars['Sign/Adv_Net_L2'])
        scalars['Sign/Model_Net_L2_Cumulative'] = self.cum_net_mov
        if self.writer:
            for name, v in scalars.items():
                self.writer.add_scalar(name, v, cur_round)
        return scalars
