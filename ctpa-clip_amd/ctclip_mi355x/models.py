"""Constructors mirroring ct_clip/pretrained_model.py:17-42 (CTViT + BERT-base + CTCLIP)."""
from __future__ import annotations

from .bert import BertConfig, BertModel
from .ct_clip import CTCLIP
from .ctvit import CTViT
from .visual_ssl import VisualSSLHead

BASE_VIT = dict(dim=512, codebook_size=8192, image_size=480, patch_size=20, temporal_patch_size=10,
                spatial_depth=4, temporal_depth=4, dim_head=32, heads=8)


def build_ctclip(vit=None, bert=None, dim_latent=512, frames=240, **loss_options):
    """CT-CLIP as the reference assembles it.  ``vit`` = CTViT kwargs (default: base),
    ``bert`` = BertConfig (default: BERT-base as CXR-BERT-specialized).  The flattened image
    embedding width follows from the ViT grid: (image/patch)^2 * dim (ct_clip.py:724,740).
    ``loss_options``: CTCLIP's decoupled_contrastive_learning / extra_latent_projection /
    multiview_loss_weight (default: the reference configuration, all off / 0.1) and
    use_all_token_embeds (the fine-grained token-wise loss: to_visual_latent then projects one
    spatial token, so its input width is the ViT token width); ``visual_ssl=True`` or a dict of
    ``VisualSSLHead`` options builds the SimSiam head on the raw image latents (with
    ``image_ssl_loss_weight``)."""
    vk = dict(BASE_VIT)
    vk.update(vit or {})
    loss_options = dict(loss_options)
    all_tokens = bool(loss_options.pop('use_all_token_embeds', False))
    # visual_ssl=True or a dict of VisualSSLHead options: the SimSiam head on the raw image latents
    head = loss_options.pop('visual_ssl', None)
    if head is True or isinstance(head, dict):
        head = VisualSSLHead(dim_latent, **(head if isinstance(head, dict) else {}))
    if head is not None and head is not False:
        loss_options['visual_ssl'] = head
    image_encoder = CTViT(**vk, use_vgg_and_gan=False)
    text_encoder = BertModel(bert or BertConfig())
    grid = vk['image_size'] // vk['patch_size']
    dim_image = vk['dim'] if all_tokens else grid * grid * vk['dim']
    return CTCLIP(image_encoder=image_encoder, text_encoder=text_encoder,
                  dim_text=text_encoder.config.hidden_size, dim_image=dim_image, dim_latent=dim_latent,
                  **{'extra_latent_projection': False, **loss_options}, use_mlm=False,
                  downsample_image_embeds=False, use_all_token_embeds=all_tokens)


def set_finetune_trainable(model):
    """ct_clip/fine_tuning_ctclip.py:6-14: freeze all, unfreeze the visual and text transformers."""
    for p in model.parameters():
        p.requires_grad = False
    for p in model.visual_transformer.parameters():
        p.requires_grad = True
    for p in model.text_transformer.parameters():
        p.requires_grad = True
    # parameters that exist in the reference's state_dict but never receive a gradient on the
    # contrastive path (ct_clip/ctvit.py:162-167,189-197; attention.py:114,117): keep them out of
    # the optimiser arena, exactly as DDP(find_unused_parameters=True) would skip them.
    vt = model.visual_transformer
    for mod in (vt.to_patch_emb_first_frame, vt.to_pixels_first_frame, vt.to_pixels):
        for p in mod.parameters():
            p.requires_grad = False
    for tr in (vt.enc_spatial_transformer, vt.enc_temporal_transformer):
        for _, attn, _, _ in tr.layers:
            attn.null_kv.requires_grad = False
            attn.context_norm.gamma.requires_grad = False
    for p in model.text_transformer.pooler.parameters():
        p.requires_grad = False
    return model
