"""rlr_amd — an MI355X-native federated-learning simulator with the Robust
Learning Rate (RLR) backdoor defense.

Re-implements, MI355X-first, the capabilities of the AAAI-2021 reference
`TinfoilHat0/Defending-Against-Backdoors-with-Robust-Learning-Rate`
(see SURVEY.md): federated training of K agents under pixel-pattern trojan
attacks, with FedAvg / coordinate-median / sign aggregation modulated by the
per-parameter robust-learning-rate sign vote.  Build addition: the
coordinate-wise trimmed mean (--aggr trmean, Yin et al. 2018), sharing one
LDS sorting-network kernel family with the median at more than 64 sampled
agents, Krum / Multi-Krum (--aggr krum, Blanchard et al. 2017) on an
fp64 MFMA pairwise-distance kernel, the geometric median / RFA
(--aggr geomed, Pillutla et al.) on a fused Weiszfeld distance kernel, and
Bulyan (--aggr bulyan, El Mhamdi et al. 2018), iterated Krum followed by a
trimmed mean around the median on a fused select-and-trim kernel; in
front of every rule, server-side norm clipping (--server_clip, Sun et al.)
on a streaming row-norm kernel, and the boosted model-replacement attack
(--attack_boost, Bagdasaryan et al.) it is the baseline defence against.

Architecture (nothing here is a port):
  * one process per GPU; sampled agents are sharded contiguously across
    ranks; per-agent update vectors are all-gathered over RCCL/xGMI and the
    aggregation runs redundantly (deterministically) on every rank
    (reference: a single-process Python dict, federated.py:67-74).
  * model parameters / grads / momentum live in flat device buffers (module
    params are views), so pack/unpack (reference agent.py:35,63) is free and
    the clip+SGD step and PGD projection are fused HIP kernels.
  * the hot ops (conv/linear fwd+bwd, relu/pool/dropout, CE loss, the
    aggregation rules, trojan injection, eval reductions) are hand-written
    HIP/CDNA4 kernels in rlr_amd/ops/csrc, dispatched on CUDA(HIP) tensors;
    the plain-PyTorch path exists only for GPU-less CI.
"""

__version__ = "0.1.0"
