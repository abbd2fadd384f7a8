"""Alphafold2 model shell: embeddings, templates, extra-MSA, recycling,
Evoformer trunk, prediction heads, IPA structure module.

Capability parity: reference alphafold2.py:469-905 — same constructor
kwargs, same forward kwargs, same state-dict layout, same return
contract.  Deliberate fixes over the reference (documented, SURVEY.md
§2.1 bug list):
  * missing-msa/embedds error is a proper ValueError (ref :711 raises an
    undefined `Error` name);
  * the extra-MSA path embeds `extra_msa` (ref :790 embeds `msa`) and
    defaults its mask from `extra_msa` (ref builds a 4-dim mask);
  * output coords are actually cast back to the input dtype (ref :893
    discards the cast result);
  * ReturnValues declares the angle-logit fields it receives.
"""
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from .. import constants
from .. import ops
from ..ops.fused_modules import FusedLayerNorm
from ..geometry.backend import torch_default_dtype
from ..mlm import MLM
from .evoformer import (  # noqa: F401 -- module-level surface parity
    Always, Attention, AxialAttention, Evoformer, EvoformerBlock,
    FeedForward, GEGLU, MsaAttentionBlock, OuterMean,
    PairwiseAttentionBlock, TriangleMultiplicativeModule, cast_tuple,
    default, exists, init_zero_,
)
from .ipa import IPABlock
from .quaternion import quaternion_multiply, quaternion_to_matrix


@dataclass
class Recyclables:
    coords: torch.Tensor
    single_msa_repr_row: torch.Tensor
    pairwise_repr: torch.Tensor


@dataclass
class ReturnValues:
    distance: Optional[torch.Tensor] = None
    theta: Optional[torch.Tensor] = None
    phi: Optional[torch.Tensor] = None
    omega: Optional[torch.Tensor] = None
    theta_logits: Optional[torch.Tensor] = None
    phi_logits: Optional[torch.Tensor] = None
    omega_logits: Optional[torch.Tensor] = None
    msa_mlm_loss: Optional[torch.Tensor] = None
    recyclables: Optional[Recyclables] = None


class Alphafold2(nn.Module):
    def __init__(
        self,
        *,
        dim,
        max_seq_len=2048,
        depth=6,
        heads=8,
        dim_head=64,
        max_rel_dist=32,
        num_tokens=constants.NUM_AMINO_ACIDS,
        num_embedds=constants.NUM_EMBEDDS_TR,
        max_num_msas=constants.MAX_NUM_MSA,
        max_num_templates=constants.MAX_NUM_TEMPLATES,
        extra_msa_evoformer_layers=4,
        attn_dropout=0.,
        ff_dropout=0.,
        templates_dim=32,
        templates_embed_layers=4,
        templates_angles_feats_dim=55,
        predict_angles=False,
        symmetrize_omega=False,
        predict_coords=False,
        structure_module_type='ipa',
        structure_module_depth=4,
        structure_module_heads=1,
        structure_module_dim_head=4,
        structure_module_refinement_iters=None,  # alias for depth
        disable_token_embed=False,
        mlm_mask_prob=0.15,
        mlm_random_replace_token_prob=0.1,
        mlm_keep_token_same_prob=0.1,
        mlm_exclude_token_ids=(0,),
        recycling_distance_buckets=32,
        reversible=False,
        checkpoint_blocks=True,
    ):
        super().__init__()
        self.dim = dim

        # token embedding
        self.token_emb = nn.Embedding(num_tokens + 1, dim) \
            if not disable_token_embed else Always(0)
        self.to_pairwise_repr = nn.Linear(dim, dim * 2)
        self.disable_token_embed = disable_token_embed

        # relative positional embedding (clamped |i - j|)
        self.max_rel_dist = max_rel_dist
        self.pos_emb = nn.Embedding(max_rel_dist * 2 + 1, dim)

        # extra-MSA evoformer (global column attention)
        self.extra_msa_evoformer = Evoformer(
            dim=dim,
            depth=extra_msa_evoformer_layers,
            seq_len=max_seq_len,
            heads=heads,
            dim_head=dim_head,
            attn_dropout=attn_dropout,
            ff_dropout=ff_dropout,
            global_column_attn=True,
            checkpoint_blocks=checkpoint_blocks,
        )

        # template embedding
        self.to_template_embed = nn.Linear(templates_dim, dim)
        self.templates_embed_layers = templates_embed_layers

        self.template_pairwise_embedder = PairwiseAttentionBlock(
            dim=dim, dim_head=dim_head, heads=heads, seq_len=max_seq_len)

        self.template_pointwise_attn = Attention(
            dim=dim, dim_head=dim_head, heads=heads, dropout=attn_dropout)

        self.template_angle_mlp = nn.Sequential(
            nn.Linear(templates_angles_feats_dim, dim),
            nn.GELU(),
            nn.Linear(dim, dim),
        )

        # angle heads
        self.predict_angles = predict_angles
        self.symmetrize_omega = symmetrize_omega
        if predict_angles:
            self.to_prob_theta = nn.Linear(dim, constants.THETA_BUCKETS)
            self.to_prob_phi = nn.Linear(dim, constants.PHI_BUCKETS)
            self.to_prob_omega = nn.Linear(dim, constants.OMEGA_BUCKETS)

        # projection for precomputed LM embeddings
        self.embedd_project = nn.Linear(num_embedds, dim)

        # main trunk (reversible = O(1)-activation execution mode)
        if reversible:
            from .reversible import make_reversible_evoformer
            self.net = make_reversible_evoformer(
                dim=dim,
                depth=depth,
                seq_len=max_seq_len,
                heads=heads,
                dim_head=dim_head,
                attn_dropout=attn_dropout,
                ff_dropout=ff_dropout,
            )
        else:
            self.net = Evoformer(
                dim=dim,
                depth=depth,
                seq_len=max_seq_len,
                heads=heads,
                dim_head=dim_head,
                attn_dropout=attn_dropout,
                ff_dropout=ff_dropout,
                checkpoint_blocks=checkpoint_blocks,
            )

        # MSA self-supervision
        self.mlm = MLM(
            dim=dim,
            num_tokens=num_tokens,
            mask_id=num_tokens,  # last embedding row doubles as mask token
            mask_prob=mlm_mask_prob,
            keep_token_same_prob=mlm_keep_token_same_prob,
            random_replace_token_prob=mlm_random_replace_token_prob,
            exclude_token_ids=mlm_exclude_token_ids,
        )

        # distogram head (on symmetrized pair rep)
        self.to_distogram_logits = nn.Sequential(
            FusedLayerNorm(dim),
            nn.Linear(dim, constants.DISTOGRAM_BUCKETS),
        )

        # structure module: 'ipa' (default, reference-layout compatible)
        # or native equivariant alternatives 'egnn' / 'se3'
        assert structure_module_type in ('ipa', 'egnn', 'se3'), \
            "structure_module_type must be 'ipa', 'egnn' or 'se3'"
        if structure_module_refinement_iters is not None:
            structure_module_depth = structure_module_refinement_iters
        self.predict_coords = predict_coords
        self.structure_module_type = structure_module_type
        self.structure_module_depth = structure_module_depth

        self.msa_to_single_repr_dim = nn.Linear(dim, dim)
        self.trunk_to_pairwise_repr_dim = nn.Linear(dim, dim)

        if structure_module_type == 'ipa':
            with torch_default_dtype(torch.float32):
                self.ipa_block = IPABlock(
                    dim=dim,
                    heads=structure_module_heads,
                )
                self.to_quaternion_update = nn.Linear(dim, 6)

            init_zero_(self.ipa_block.attn.to_out)

            self.to_points = nn.Linear(dim, 3)
        else:
            from .equivariant import EquivariantStructureModule
            with torch_default_dtype(torch.float32):
                self.structure_module = EquivariantStructureModule(
                    dim, depth=structure_module_depth,
                    kind=structure_module_type,
                    heads=max(structure_module_heads, 4),
                    dim_head=max(structure_module_dim_head, 16))

        # per-residue confidence head
        self.lddt_linear = nn.Linear(dim, 1)

        # recycling
        self.recycling_msa_norm = FusedLayerNorm(dim)
        self.recycling_pairwise_norm = FusedLayerNorm(dim)
        self.recycling_distance_embed = nn.Embedding(
            recycling_distance_buckets, dim)
        self.recycling_distance_buckets = recycling_distance_buckets

    def forward(
        self,
        seq,
        msa=None,
        mask=None,
        msa_mask=None,
        extra_msa=None,
        extra_msa_mask=None,
        seq_index=None,
        seq_embed=None,
        msa_embed=None,
        templates_feats=None,
        templates_mask=None,
        templates_angles=None,
        embedds=None,
        recyclables=None,
        return_trunk=False,
        return_confidence=False,
        return_recyclables=False,
        return_aux_logits=False,
    ):
        assert not (self.disable_token_embed and not exists(seq_embed)), \
            'sequence embedding must be supplied if token embedding is disabled'
        assert not (self.disable_token_embed and not exists(msa_embed)), \
            'msa embedding must be supplied if token embedding is disabled'

        # without an MSA, treat the primary sequence as a single-row MSA
        if not exists(msa) and not exists(embedds):
            msa = seq[:, None, :]
            msa_mask = mask[:, None, :] if exists(mask) else None

        if exists(msa):
            assert msa.shape[-1] == seq.shape[-1], \
                'sequence length of MSA and primary sequence must be the same'

        b, n = seq.shape[:2]
        device = seq.device

        # embed main sequence
        x = self.token_emb(seq)
        if exists(seq_embed):
            x = x + seq_embed

        # MLM corruption (training only)
        original_msa = msa
        replaced_msa_mask = None
        if self.training and exists(msa):
            msa_mask = default(msa_mask, lambda: torch.ones_like(msa).bool())
            msa, replaced_msa_mask = self.mlm.noise(msa, msa_mask)

        # embed MSA (or precomputed LM embeddings)
        if exists(msa):
            m = self.token_emb(msa)
            if exists(msa_embed):
                m = m + msa_embed
            m = m + x[:, None, :, :]  # broadcast single repr onto rows
            msa_mask = default(msa_mask, lambda: torch.ones_like(msa).bool())
        elif exists(embedds):
            m = self.embedd_project(embedds)
            msa_mask = default(
                msa_mask, lambda: torch.ones_like(embedds[..., -1]).bool())
        else:
            raise ValueError('either MSA or embedds must be given')

        # pairwise representation: outer sum + relative position
        # embedding, built in ONE fused pass (K13) when on GPU
        x_left, x_right = self.to_pairwise_repr(x).chunk(2, dim=-1)
        x_mask = mask[:, :, None] * mask[:, None, :] if exists(mask) else None

        seq_index = default(
            seq_index, lambda: torch.arange(n, device=device))
        seq_rel_dist = seq_index[None, :, None] - seq_index[None, None, :]
        seq_rel_dist = seq_rel_dist.clamp(
            -self.max_rel_dist, self.max_rel_dist) + self.max_rel_dist
        x = ops.pair_rep_build(x_left.contiguous(), x_right.contiguous(),
                               self.pos_emb.weight, seq_rel_dist)

        # recycling inputs
        if exists(recyclables):
            m = torch.cat([
                (m[:, 0] + self.recycling_msa_norm(
                    recyclables.single_msa_repr_row)).unsqueeze(1),
                m[:, 1:]], dim=1)
            x = x + self.recycling_pairwise_norm(recyclables.pairwise_repr)

            boundaries = torch.linspace(
                2, 20, steps=self.recycling_distance_buckets, device=device)
            discretized = ops.distance_buckets(
                recyclables.coords, boundaries[:-1])
            x = x + self.recycling_distance_embed(discretized)

        # templates
        if exists(templates_feats):
            _, num_templates, *_ = templates_feats.shape

            t = self.to_template_embed(templates_feats)
            t_mask_crossed = templates_mask[:, :, :, None] \
                * templates_mask[:, :, None, :]

            t = t.reshape(-1, *t.shape[2:])
            t_mask_crossed = t_mask_crossed.reshape(
                -1, *t_mask_crossed.shape[2:])

            for _ in range(self.templates_embed_layers):
                t = self.template_pairwise_embedder(t, mask=t_mask_crossed)

            t = t.reshape(b, num_templates, *t.shape[1:])
            t_mask_crossed = t_mask_crossed.reshape(
                b, num_templates, *t_mask_crossed.shape[1:])

            # pool over templates with pointwise cross-attention per (i, j)
            x_mask_point = x_mask.reshape(b * n * n, 1) \
                if exists(x_mask) else None
            t_mask_point = t_mask_crossed.permute(0, 2, 3, 1).reshape(
                b * n * n, num_templates)

            # on the GPU the pointwise kernels (K5) take x, t and the
            # masks in the layouts they have; None = the gate declined
            template_pooled = None
            if x.is_cuda:
                template_pooled = \
                    self.template_pointwise_attn.pointwise_context(
                        x.reshape(b, n * n, self.dim),
                        t.reshape(b, num_templates, n * n, self.dim),
                        query_mask=x_mask.reshape(b, n * n)
                        if exists(x_mask) else None,
                        key_mask=t_mask_crossed.reshape(
                            b, num_templates, n * n))
            if exists(template_pooled):
                template_pooled = template_pooled.reshape(
                    b * n * n, 1, self.dim)
            else:
                x_point = x.reshape(b * n * n, 1, self.dim)
                t_point = t.permute(0, 2, 3, 1, 4).reshape(
                    b * n * n, num_templates, self.dim)
                template_pooled = self.template_pointwise_attn(
                    x_point,
                    context=t_point,
                    mask=x_mask_point,
                    context_mask=t_mask_point,
                )

            template_pooled_mask = (
                t_mask_point.sum(dim=-1) > 0)[:, None, None]
            template_pooled = template_pooled * template_pooled_mask

            x = x + template_pooled.reshape(b, n, n, self.dim)

        # template torsion-angle features join the MSA rows
        if exists(templates_angles):
            t_angle_feats = self.template_angle_mlp(templates_angles)
            m = torch.cat((m, t_angle_feats), dim=1)
            msa_mask = torch.cat((msa_mask, templates_mask), dim=1)

        # under autocast, run the trunk streams natively in the compute
        # dtype: embedding/positional additions above are fp32 and would
        # otherwise drag every residual/LN/elementwise op in the trunk
        # through fp32 (2x HBM traffic) plus per-Linear input casts
        if torch.is_autocast_enabled() and x.is_cuda:
            ac = torch.get_autocast_dtype('cuda')
            x = x.to(ac)
            m = m.to(ac)

        # extra MSAs run through their own evoformer with tied-query
        # column attention (fix over ref :790 which embeds `msa` here)
        if exists(extra_msa):
            extra_m = self.token_emb(extra_msa)
            extra_msa_mask = default(
                extra_msa_mask, lambda: torch.ones_like(extra_msa).bool())
            x, extra_m = self.extra_msa_evoformer(
                x, extra_m, mask=x_mask, msa_mask=extra_msa_mask)

        # main trunk
        x, m = self.net(x, m, mask=x_mask, msa_mask=msa_mask)

        ret = ReturnValues()

        # theta and phi come from the un-symmetrized pair rep
        if self.predict_angles:
            ret.theta_logits = self.to_prob_theta(x)
            ret.phi_logits = self.to_prob_phi(x)

        trunk_embeds = (x + x.transpose(1, 2)) * 0.5  # symmetrize
        ret.distance = self.to_distogram_logits(trunk_embeds)

        if self.training and exists(original_msa):
            num_msa = original_msa.shape[1]
            ret.msa_mlm_loss = self.mlm(
                m[:, :num_msa], original_msa, replaced_msa_mask)

        if self.predict_angles:
            omega_input = trunk_embeds if self.symmetrize_omega else x
            ret.omega_logits = self.to_prob_omega(omega_input)

        if not self.predict_coords or return_trunk:
            return ret

        # single / pairwise projections for structure refinement
        single_msa_repr_row = m[:, 0]
        single_repr = self.msa_to_single_repr_dim(single_msa_repr_row)
        pairwise_repr = self.trunk_to_pairwise_repr_dim(x)

        original_dtype = single_repr.dtype
        single_repr = single_repr.float()
        pairwise_repr = pairwise_repr.float()

        if self.structure_module_type != 'ipa':
            # equivariant refinement (EGNN / SE3-style), fp32
            with torch_default_dtype(torch.float32):
                start = recyclables.coords.float() \
                    if exists(recyclables) else None
                single_repr, coords = self.structure_module(
                    single_repr, pairwise_repr, mask=mask, coords=start)
            coords = coords.type(original_dtype)

            if return_recyclables:
                rec = map(torch.detach,
                          (coords, single_msa_repr_row, pairwise_repr))
                ret.recyclables = Recyclables(*rec)
            if return_aux_logits:
                return coords, ret
            if return_confidence:
                return coords, self.lddt_linear(single_repr.float())
            return coords

        # iterative IPA refinement in fp32 (equivariance)
        with torch_default_dtype(torch.float32):
            quaternions = torch.tensor(
                [1., 0., 0., 0.], device=device).expand(b, n, 4)
            translations = torch.zeros((b, n, 3), device=device)

            for i in range(self.structure_module_depth):
                is_last = i == (self.structure_module_depth - 1)

                # rotation gradients detached except on the final
                # iteration (mirrors DeepMind folding)
                rotations = quaternion_to_matrix(quaternions)
                if not is_last:
                    rotations = rotations.detach()

                single_repr = self.ipa_block(
                    single_repr,
                    mask=mask,
                    pairwise_repr=pairwise_repr,
                    rotations=rotations,
                    translations=translations,
                )

                # 6-dof update: quaternion (3, w implicitly 1) + translation
                quaternion_update, translation_update = \
                    self.to_quaternion_update(single_repr).chunk(2, dim=-1)
                quaternion_update = F.pad(quaternion_update, (1, 0), value=1.)

                quaternions = quaternion_multiply(
                    quaternions, quaternion_update)
                translations = translations + torch.einsum(
                    'b n c, b n c r -> b n r', translation_update, rotations)

            points_local = self.to_points(single_repr)
            rotations = quaternion_to_matrix(quaternions)
            coords = torch.einsum(
                'b n c, b n c d -> b n d', points_local, rotations) \
                + translations

        coords = coords.type(original_dtype)

        if return_recyclables:
            rec_coords, rec_single, rec_pair = map(
                torch.detach, (coords, single_msa_repr_row, pairwise_repr))
            ret.recyclables = Recyclables(rec_coords, rec_single, rec_pair)

        if return_aux_logits:
            return coords, ret

        if return_confidence:
            return coords, self.lddt_linear(single_repr.float())

        return coords
