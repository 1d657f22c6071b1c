from .decode_head import DynamicBaseDecodeHead  # noqa: F401
from .dynamic_aspp_head import (DynamicASPPHead, DynamicASPPModule,  # noqa: F401
                                DynamicDepthwiseSeparableASPPHead,
                                DynamicDepthwiseSeparableASPPModule)
from .dynamic_fcn_head import DynamicFCNHead  # noqa: F401
from .dynamic_ocr_head import DynamicObjectAttentionBlock, DynamicOCRHead  # noqa: F401
from .dynamic_psp_head import DynamicPPM, DynamicPSPHead  # noqa: F401
from .dynamic_uper_head import DynamicUPerHead  # noqa: F401
from .dynamic_segformer_head import DynamicSegformerHead  # noqa: F401
