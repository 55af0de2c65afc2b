from .seal_utils import SealAnchorMapper, SealBBoxMapper, SealBrushMapper, get_seal_mapper, pil_image_loader  # noqa: F401
from .renderer import SealTeacherMixin, make_teacher, make_student  # noqa: F401
from .trainer import GraphedSealTrainer, SealTrainer, get_trainer, sample_points  # noqa: F401
from .provider import SealDataset, SealRandomDataset  # noqa: F401
from .preview import SealSession  # noqa: F401
