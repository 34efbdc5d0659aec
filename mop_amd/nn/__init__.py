"""nn.Module surface mirroring `mop.models` of the reference (names as in mop/models/__init__.py)."""
from .attention_variants import (BaselineMSA, CrossViewMixerMSA, EdgewiseGateHead,  # noqa: F401
                                 EdgewiseMSA, MultiHopMSA, UnifiedMSA)
from .components import (MLP, MSA, Block, DropPath, FuseExcInh, Kernels3, PatchEmbed,  # noqa: F401
                         ViewsLinear, ViTEncoder)
from .quartet_attn_patch import CausalSelfAttention, TransformerConfig  # noqa: F401
from .vit_mop import ViT_MoP  # noqa: F401
from .whisper_mop import (DecoderBlock, EncodedAudio, EncoderBlock, FuseExcInh2D, Kernels2D, MoP2D,  # noqa: F401
                          MultiheadCrossAttention, MultiheadSelfAttention, ViewsConv2D, WhisperConfig, WhisperDecodeCache, WhisperMoP,
                          create_whisper_baseline, create_whisper_mop, LogMelFrontend, RuledDecoding, TokenAlignment, Transcript,
                          DecodeStats, TranscribeLog, WordAlignment, TranscriptWords, LanguageDetection, Resample,
                          ResampledLogMelFrontend)
from ..ops import LogitRules, LanguageTokens, RepeatRules, WordRules  # noqa: F401  (the rule sets of WhisperMoP.with_logit_rules, the language tokens of detect_language, the word table of align_words)
from .vit_edgewise import BlockEdgewise, ViTEdgewise  # noqa: F401
# GPT line (mop/models/gpt_mop.py).  The Quartet MLP / Block / TinyTransformerLM live in .quartet_attn_patch; MLP and Block here stay
# the ViT ones, as in the reference's mop.models.
from .gpt_mop import (FuseExcInh1D, GPT_MoP, Kernels1D, MoPBlock, ViewsLinear1D, create_gpt_baseline,  # noqa: F401
                      create_gpt_mop, create_gpt_quartet)
from .quartet_attn_patch import TinyTransformerLM  # noqa: F401
